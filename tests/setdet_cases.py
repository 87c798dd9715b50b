"""Shared by the set-prediction detector stage's tests (not a test module): the cases, a PyTorch oracle written from the
contract of include/gsraster.h (GsrSetDetSpec) and the host build of csrc/gsr_setdet.h (tests/host_math/setdet_host.cpp).

The oracle is vectorised torch code whose gradient comes from torch.autograd, so it shares nothing with the hand-written
backward.  Run in float64 it is the reference; the same code in float32 on the CPU is the yardstick: a float32 evaluation
of the same formulas in another summation order and with other exp / log roundings.  For a compared tensor q,
err(q) = max|q - q64| / max(max|q64|, 1e-30); the host build and the kernels may have at most FACTOR = 4 times the
yardstick's err for the same case and tensor, with a floor of 2^-22 and never more than the project's 1e-3 gradient
tolerance (detloss_cases.bound, reused).

The oracle's matcher (solve_assignment) is its own: successive shortest paths found by Bellman-Ford relaxation of the
residual graph in float64, without dual potentials -- not the algorithm of gsr_setdet.h.  It is cross-checked against all
permutations on small sizes and against scipy where scipy imports.

Integer results (match, tgt) of a float32 evaluation equal the oracle's only while the optimum is unique by more than
float32 rounding can move a sum of cost entries, so the seeds are chosen such that (asserted by the CPU tests, never
skipped):
  * for every image the best assignment that differs from the optimum costs more by > 1e-3 (found by forbidding each
    matched pair in turn and re-solving); float32 cost entries differ from float64 by about 2e-6, at most 1e-4 over 32 rows,
  * for the output stage every score is further than 1e-4 from conf_thr and every class maximum leads the runner-up by
    more than 1e-4 relative.
python tests/setdet_cases.py searches the seeds and asserts the committed ones.

Where the margins are given up on purpose the inputs are hand-made from values that are exact in float32 (tie_inputs,
kink_inputs, score_inputs), so that equal stays equal in any precision and the contract's tie rules decide; the checks that
the host and the device tests share on them (check_tie, check_with_match_frozen, exact_score_expectations, check_poisoned)
live here too.
"""
import ctypes
import itertools
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from detloss_cases import bound, err  # noqa: F401  (the project's bound, shared)
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM = os.path.join(ROOT, "tests", "host_math")
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
FRAME = (640.0, 480.0)                      # img_w, img_h
C_CLASS, C_L1, C_GIOU = 1.0, 5.0, 2.0
W_CE, W_L1, W_GIOU, EOS = 1.0, 5.0, 2.0, 0.1
CONF_THR = 0.7
COMPARED = ("loss", "grad_logits", "grad_boxes")
GAP_MATCH, GAP_SCORE, GAP_LEAD = 1e-3, 1e-4, 1e-4


class Case(NamedTuple):
    id: str
    B: int
    Q: int
    C: int
    M: int
    kind: str = "plain"          # plain | ragged | contested | nogt | saturated
    seed: int = 0


# the seeds satisfy the margin conditions and the properties test_the_cases_cover_what_they_claim asserts
CASES = [
    Case("one", 1, 1, 1, 1, seed=0),
    Case("tiny", 2, 8, 3, 2, seed=0),
    Case("ragged", 3, 100, 91, 5, kind="ragged", seed=0),
    Case("contested", 2, 16, 4, 6, kind="contested", seed=0),
    Case("full-rows", 1, 32, 5, 32, seed=0),
    Case("no-gt", 2, 8, 3, 2, kind="nogt", seed=0),
    Case("saturated", 2, 8, 3, 2, kind="saturated", seed=0),
    Case("wide", 2, 900, 91, 8, seed=0),
    # the edges of what the kernels add to the scalar source: wave and workgroup widths of the match's column dealing and of
    # the row of logits, B * Q that is no multiple of the cost kernel's four queries, the stride loops' second trip, the maxima
    Case("q63", 1, 63, 62, 5, seed=0),             # one wave of columns, one short lane; a row of 63 logits
    Case("q64-n64", 1, 64, 63, 7, seed=0),         # exactly one wave of columns; a row of exactly 64 logits
    Case("q65-n65", 2, 65, 64, 9, seed=0),         # one column and one logit in the second wave; B * Q = 130
    Case("q255", 1, 255, 3, 32, seed=0),           # all four waves, the last lane idle; MAX_ROWS against a wide Q
    Case("q256", 1, 256, 5, 31, seed=0),           # every lane exactly one column
    Case("q257", 3, 257, 7, 32, seed=1),           # one column on the second trip of the stride loop; B * Q = 771
    Case("odd-square", 1, 5, 2, 5, seed=0),        # Q = M; a cost workgroup with three idle waves
    Case("many-images", 257, 3, 2, 2, seed=0),     # block_matched's second trip; 257 match workgroups
    Case("limits", 1, 1024, 1024, 32, seed=0),     # every maximum at once: 1025 logits a row, 1025 term blocks
]
BY_ID = {c.id: c for c in CASES}
TERM_TILE = 1024                                   # logits per workgroup of k_setdet_terms (gsr_setdet.hip.h)
# what the edge cases claim beyond the margins (covers): B * Q mod 4, and which stride loop takes a second trip
EDGE_CLAIMS = {"q63": dict(bq_mod4=3), "q64-n64": dict(bq_mod4=0), "q65-n65": dict(bq_mod4=2), "q255": dict(bq_mod4=3),
               "q256": dict(bq_mod4=0), "q257": dict(bq_mod4=3), "odd-square": dict(bq_mod4=1),
               "many-images": dict(bq_mod4=3, images_above=256), "limits": dict(bq_mod4=0, term_blocks_above=256)}


def term_blocks(c: Case) -> int:
    return (c.B * c.Q * (c.C + 1) + TERM_TILE - 1) // TERM_TILE


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_inputs(c: Case):
    """-> (logits float32 [B,Q,C+1], boxes float32 [B,Q,4] cx cy w h normalised, gt_boxes float32 [B,M,4] x1 y1 x2 y2 in pixels
    of FRAME, gt_cls int32 [B,M]) as numpy arrays.  Half of the queries sit near one of the image's boxes (jittered) so that
    rows compete for them; a third of the queries carry one confident class so that the output stage keeps some."""
    rng = np.random.default_rng(9100 + 977 * c.seed + 31 * c.Q + 7 * c.M + c.C)
    W, H = FRAME
    gtn = np.zeros((c.B, c.M, 4))
    for b in range(c.B):
        if c.kind == "contested":
            base = np.array([rng.uniform(0.4, 0.6), rng.uniform(0.4, 0.6), rng.uniform(0.25, 0.4), rng.uniform(0.25, 0.4)])
            gtn[b] = base * rng.uniform(0.97, 1.03, (c.M, 4))                  # near-duplicates of one box
        else:
            gtn[b, :, :2] = rng.uniform(0.25, 0.75, (c.M, 2))
            gtn[b, :, 2:] = rng.uniform(0.1, 0.45, (c.M, 2))
    gt = np.stack([(gtn[..., 0] - gtn[..., 2] / 2) * W, (gtn[..., 1] - gtn[..., 3] / 2) * H,
                   (gtn[..., 0] + gtn[..., 2] / 2) * W, (gtn[..., 1] + gtn[..., 3] / 2) * H], axis=-1)
    cls = rng.integers(0, c.C, (c.B, c.M)).astype(np.int32)
    if c.kind == "ragged":
        cls[0, 1] = -1                                   # present rows are not contiguous
        cls[1, :] = -1                                   # one image with every row absent
        cls[2, 3] = c.C + 5                              # a class past the head's: absent as well
    if c.kind == "nogt":
        cls[:] = -1
    boxes = np.zeros((c.B, c.Q, 4))
    boxes[..., :2] = rng.uniform(0.2, 0.8, (c.B, c.Q, 2))
    boxes[..., 2:] = rng.uniform(0.08, 0.4, (c.B, c.Q, 2))
    near = max(1, c.Q // 2) if c.Q > 1 else 1
    for b in range(c.B):
        picks = rng.permutation(c.Q)[:near]
        rows = rng.integers(0, c.M, near)
        jit = 0.12 if c.kind == "contested" else 0.25
        boxes[b, picks] = gtn[b, rows] * rng.uniform(1 - jit, 1 + jit, (near, 4))
    if c.kind == "saturated":
        logits = np.full((c.B, c.Q, c.C + 1), -80.0)
        top = rng.integers(0, c.C, (c.B, c.Q))
        np.put_along_axis(logits, top[..., None], 80.0, axis=2)               # exactly one class at +80 ...
        logits[..., c.C] = np.where(rng.uniform(0, 1, (c.B, c.Q)) < 0.5, 80.0, -80.0)   # ... "no object" at +80 or -80
        boxes[:, 0] = (0.125, 0.5, 0.25, 0.5)                                  # x1 = 0 exactly
        boxes[:, 1] = (0.875, 0.5, 0.25, 1.0)                                  # x2 = 1, y1 = 0, y2 = 1 exactly
    else:
        logits = rng.normal(0.0, 2.0, (c.B, c.Q, c.C + 1))
        sure = rng.uniform(0, 1, (c.B, c.Q)) < 1 / 3
        hot = rng.integers(0, c.C, (c.B, c.Q))
        boost = np.zeros_like(logits)
        np.put_along_axis(boost, hot[..., None], 9.0, axis=2)
        logits = logits + boost * sure[..., None]
    return logits.astype(np.float32), boxes.astype(np.float32), gt.astype(np.float32), cls


# ---- hand-made inputs: exact ties, the backward's kinks, exact scores, non-finite values ---------------------------------------
TIE_KINDS = ("identical", "block", "prototypes")
TIE_Q, TIE_C, TIE_M = 300, 3, 6
TIE_GT = (200.0, 150.0, 440.0, 330.0)              # (0.5, 0.5, 0.375, 0.375) normalised in FRAME, exactly
TIE_BLOCK = range(253, 265)                        # the cheaper block: it straddles column 256 of the match's 256 lanes
TIE_PROTO_SEED = 0                                 # the first seed whose distinct costs of a row lie > GAP_MATCH apart


def tie_inputs(kind):
    """One image whose match is decided by the tie rule alone (smallest value, lowest column among equals, rows inserted in
    order): every value is a copy, so equal pairs have equal costs bit for bit in any precision.
      identical   TIE_Q identical queries, TIE_M identical rows: the rule gives row m query m
      block       the same, but queries TIE_BLOCK carry the gt's own box: a strictly cheaper block of equal candidates whose
                  winners come from two waves, from lanes 252..255 and from the second trip of the stride loop (0, 1)
      prototypes  five (logits, box) prototypes dealt at random over the queries, six rows that are copies of two boxes with
                  classes (1, 1, 2, 1, 2, 2): equal candidates all over the columns, two pairs of identical rows
    -> (logits [1,Q,C+1], boxes [1,Q,4], gt_boxes [1,M,4], gt_cls [1,M])."""
    Q, C, M = TIE_Q, TIE_C, TIE_M
    if kind in ("identical", "block"):
        logits = np.tile(np.array([0.5, 1.0, -0.25, 0.0], np.float32), (1, Q, 1))
        boxes = np.tile(np.array([0.5, 0.5, 0.25, 0.25], np.float32), (1, Q, 1))
        if kind == "block":
            boxes[0, list(TIE_BLOCK)] = (0.5, 0.5, 0.375, 0.375)
        gt = np.tile(np.array(TIE_GT, np.float32), (1, M, 1))
        return logits, boxes, gt, np.full((1, M), 1, np.int32)
    assert kind == "prototypes"
    rng = np.random.default_rng(7300 + TIE_PROTO_SEED)
    W, H = FRAME
    p_logits = rng.normal(0.0, 2.0, (5, C + 1)).astype(np.float32)
    p_boxes = np.concatenate([rng.uniform(0.3, 0.7, (5, 2)), rng.uniform(0.1, 0.4, (5, 2))], axis=1).astype(np.float32)
    deal = rng.integers(0, 5, Q)
    two = np.concatenate([rng.uniform(0.3, 0.7, (2, 2)), rng.uniform(0.15, 0.4, (2, 2))], axis=1)
    two = np.stack([(two[:, 0] - two[:, 2] / 2) * W, (two[:, 1] - two[:, 3] / 2) * H, (two[:, 0] + two[:, 2] / 2) * W,
                    (two[:, 1] + two[:, 3] / 2) * H], axis=-1).astype(np.float32)
    gt = two[[0, 0, 0, 1, 1, 1]][None]
    return p_logits[deal][None], p_boxes[deal][None], gt, np.array([[1, 1, 2, 1, 2, 2]], np.int32)


def distinct_gap(cost_row):
    """The smallest difference between two distinct values of a row of costs (inf if all are one value)."""
    v = np.unique(np.asarray(cost_row, np.float64))
    return float(np.diff(v).min()) if len(v) > 1 else math.inf


def assignment_cost(cost, match):
    """The cost of match [M] (-1: no query) in cost [M,Q], summed exactly."""
    return math.fsum(float(cost[m, q]) for m, q in enumerate(match) if q >= 0)


KINKS = (("equal", (0.5, 0.5, 0.5, 0.5)), ("touching-right", (0.875, 0.5, 0.25, 0.5)),
         ("touching-corner", (0.875, 0.875, 0.25, 0.25)), ("disjoint", (0.125, 0.125, 0.125, 0.125)),
         ("containing", (0.5, 0.5, 0.75, 0.75)), ("inside-shared-edge", (0.375, 0.5, 0.25, 0.25)), ("zero-size", (0.5, 0.5, 0.0, 0.0)))
KINK_GT = (160.0, 120.0, 480.0, 360.0)             # (0.5, 0.5, 0.5, 0.5) normalised in FRAME, exactly
KINK_EXACT = ("equal", "inside-shared-edge", "zero-size")     # every step of their box gradient is exact in float32


def kink_inputs(only=None):
    """The hand-written GIoU / L1 backward where max, min, clamp and abs have their kinks: one gt row per image and query 0
    in an exact relation to it (KINKS, one image each; only = a name: that image alone); query 1 is a far decoy whose
    logits speak against the row's class, so the row takes query 0.  Every coordinate is a short binary fraction.
    -> (logits [B,2,3], boxes [B,2,4], gt_boxes [B,1,4], gt_cls [B,1])."""
    kinks = [k for k in KINKS if only is None or k[0] == only]
    B = len(kinks)
    logits = np.tile(np.array([[2.0, 0.0, -1.0], [-8.0, 8.0, 0.0]], np.float32), (B, 1, 1))
    boxes = np.zeros((B, 2, 4), np.float32)
    boxes[:, 0] = [k[1] for k in kinks]
    boxes[:, 1] = (0.0625, 0.9375, 0.0625, 0.0625)
    return logits, boxes, np.tile(np.array(KINK_GT, np.float32), (B, 1, 1)), np.zeros((B, 1), np.int32)


def score_inputs():
    """The output stage at exact scores: C = 2, one image, five queries -> (logits [1,5,3], boxes [1,5,4]).
      0: (1, 1, -inf)     a class tie at p = 0.5 exactly: class 0      1: (0, 2, 2)   class 1
      2: (NaN, 0, 0)      never kept                                    3: (-inf, -inf, 0)   both classes at 0
      4: (3, 3, 3)        a tie at 1/3: class 0"""
    inf, nan = np.inf, np.nan
    logits = np.array([[[1, 1, -inf], [0, 2, 2], [nan, 0, 0], [-inf, -inf, 0], [3, 3, 3]]], np.float32)
    boxes = np.array([[[0.5, 0.5, 0.25, 0.25], [0.25, 0.75, 0.5, 0.125], [0.5, 0.5, 0.5, 0.5], [0.75, 0.25, 0.125, 0.25],
                       [0.375, 0.625, 0.25, 0.75]]], np.float32)
    return logits, boxes


def poison(a, frac, rng, images=None):
    """A copy of a with a share frac of the elements (of the images named, default all) made non-finite: 40 % NaN, 30 % +inf,
    30 % -inf."""
    a = a.copy()
    bad = rng.uniform(0, 1, a.shape)
    if images is not None:
        keep = np.ones(a.shape[0], bool)
        keep[list(images)] = False
        bad[keep] = 2.0
    a[bad < frac * 0.4] = np.nan
    a[(bad >= frac * 0.4) & (bad < frac * 0.7)] = np.inf
    a[(bad >= frac * 0.7) & (bad < frac)] = -np.inf
    return a


NONFINITE_CASES = (Case("nonfinite", 3, 70, 5, 6, seed=0), BY_ID["q257"])    # image 1 of three is the poisoned one
NONFINITE_FRACS = (0.05, 0.5, 1.0)


def poisoned_inputs(c: Case, frac):
    """make_inputs(c) with the share frac of image 1's logits and boxes made non-finite -> (logits, boxes)."""
    logits, boxes, _, _ = make_inputs(c)
    rng = np.random.default_rng(4000 + int(frac * 100))
    return poison(logits, frac, rng, images=[1]), poison(boxes, frac, rng, images=[1])


def check_poisoned(who, c: Case, got, clean, gt_cls, counts):
    """got: the outputs (numpy) for poisoned_inputs(c, .), clean: for make_inputs(c), counts: the output stage's for the
    poisoned inputs.  The floats of the poisoned image are unspecified; what holds is that every index is in range, the
    match is one-to-one over exactly the present rows with tgt its inverse, every gradient element is written, and the
    other images have the clean run's bits: the normalisers are integers (matched rows, B * Q) and every present row is
    matched either way."""
    match, tgt = got["match"], got["tgt"]
    present = (gt_cls >= 0) & (gt_cls < c.C)
    assert match.min() >= -1 and match.max() < c.Q, who
    assert tgt.min() >= -1 and tgt.max() < c.M, who
    assert ((match >= 0) == present).all(), who
    for b in range(c.B):
        rows = np.nonzero(present[b])[0]
        qs = match[b][rows]
        assert len(set(qs.tolist())) == len(qs) and (tgt[b, qs] == rows).all() and (tgt[b] >= 0).sum() == len(rows), (who, b)
    assert counts.min() >= 0 and counts.max() <= c.Q, who
    for b in (0, 2):
        for k in ("match", "tgt", "grad_logits", "grad_boxes"):
            assert got[k][b].tobytes() == clean[k][b].tobytes(), f"{who}: {k} of image {b} differs from the clean run"


# ---- the oracle's matcher ---------------------------------------------------------------------------------------------------
def solve_assignment(cost, rows):
    """cost [M,Q] float64, rows: the present rows -> (row_to_col [M] with -1 for the others, the optimum's cost).
    Successive shortest augmenting paths: each new row's cheapest alternating path to a free column is found by relaxing
    all residual edges until nothing changes (Bellman-Ford; matched edges run backwards with the negated cost)."""
    cost = np.asarray(cost, np.float64)
    M, Q = cost.shape
    r2c = np.full(M, -1, np.int64)
    c2r = np.full(Q, -1, np.int64)
    done = []
    for r in rows:
        act = np.array(done + [r])
        dist_r = np.full(M, np.inf)
        dist_r[r] = 0.0
        dist_c = np.full(Q, np.inf)
        par_c = np.full(Q, -1, np.int64)
        for _ in range(2 * len(act) + 2):
            cand = dist_r[act, None] + cost[act]                               # forward edges: unmatched (row, column)
            held = r2c[act]
            cand[np.nonzero(held >= 0)[0], held[held >= 0]] = np.inf
            k = cand.argmin(0)
            best = cand[k, np.arange(Q)]
            upd = best < dist_c
            dist_c[upd] = best[upd]
            par_c[upd] = act[k[upd]]
            changed = bool(upd.any())
            for m in done:                                                      # backward edges: a held column frees its row
                nd = dist_c[r2c[m]] - cost[m, r2c[m]]
                if nd < dist_r[m]:
                    dist_r[m] = nd
                    changed = True
            if not changed:
                break
        free = np.nonzero(c2r < 0)[0]
        col = int(free[np.argmin(dist_c[free])])
        for _ in range(len(act) + 1):
            m = int(par_c[col])
            prev = int(r2c[m])
            r2c[m], c2r[col] = col, m
            if m == r:
                break
            col = prev
        done.append(r)
    total = float(sum(cost[m, r2c[m]] for m in rows))
    return r2c, total


def brute_force(cost, rows):
    cost = np.asarray(cost, np.float64)
    best, arg = math.inf, None
    for perm in itertools.permutations(range(cost.shape[1]), len(rows)):
        t = sum(cost[m, q] for m, q in zip(rows, perm))
        if t < best:
            best, arg = t, perm
    return arg, best


def greedy_cost(cost, rows):
    """Every row in ascending order takes its cheapest free column."""
    cost = np.asarray(cost, np.float64)
    taken, total = set(), 0.0
    for m in rows:
        q = min((q for q in range(cost.shape[1]) if q not in taken), key=lambda q: cost[m, q])
        taken.add(q)
        total += cost[m, q]
    return total


def match_gap(cost, rows, r2c, total):
    """The cost by which the best assignment that differs from the optimum exceeds it: forbid each matched pair in turn."""
    gap = math.inf
    for m in rows:
        alt = np.array(cost, np.float64)
        alt[m, r2c[m]] = 1e9
        a2, t2 = solve_assignment(alt, rows)
        if a2[m] != r2c[m]:                                                     # (Q = M = 1: no other assignment exists)
            gap = min(gap, t2 - total)
    return gap


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def xyxy(b):
    return torch.stack([b[..., 0] - 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 0] + 0.5 * b[..., 2],
                        b[..., 1] + 0.5 * b[..., 3]], dim=-1)


def giou(a, b):
    """a, b: [..., 4] x1 y1 x2 y2, broadcastable."""
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    inter = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp(min=0) * \
            (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp(min=0)
    union = area_a + area_b - inter
    encl = (torch.maximum(a[..., 2], b[..., 2]) - torch.minimum(a[..., 0], b[..., 0])).clamp(min=0) * \
           (torch.maximum(a[..., 3], b[..., 3]) - torch.minimum(a[..., 1], b[..., 1])).clamp(min=0)
    return inter / union - (encl - union) / encl


def _tensor(a):
    return a.detach() if torch.is_tensor(a) else torch.tensor(np.array(a))       # a copy: the cached inputs are read-only


def normalise_gt(gt_boxes, frame, dtype):
    W, H = frame
    g = gt_boxes.to(dtype)
    return torch.stack([(g[..., 0] + g[..., 2]) * 0.5 / W, (g[..., 1] + g[..., 3]) * 0.5 / H, (g[..., 2] - g[..., 0]) / W,
                        (g[..., 3] - g[..., 1]) / H], dim=-1)


def oracle(logits, boxes, gt_boxes, gt_cls, dtype=torch.float64, frame=FRAME, costs=(C_CLASS, C_L1, C_GIOU),
           w=(W_CE, W_L1, W_GIOU), eos=EOS, want_grad=True, device="cpu", want_gap=False, solver=None, match=None):
    """The contract of include/gsraster.h in torch.  logits / boxes may be tensors that require grad (then `total` is
    returned attached and no backward is run here).  -> dict(match, tgt, cost, loss[4], total, grad_logits, grad_boxes,
    gap_match, greedy_excess).  solver (default solve_assignment): what matches one image's rows on the host.
    match [B,M] (-1: no query): the match is taken from there and no solver runs -- the loss and the gradients of a frozen
    match, what the contract's gradient holds constant."""
    f32 = lambda v: float(np.float32(v))                                          # the spec's fields are float32
    frame, costs, w, eos = tuple(map(f32, frame)), tuple(map(f32, costs)), tuple(map(f32, w)), f32(eos)
    attached = torch.is_tensor(logits) and logits.requires_grad
    if attached:
        x, bx = logits.to(dtype), boxes.to(dtype)
    else:
        x = _tensor(logits).to(device=device, dtype=dtype).clone().requires_grad_(want_grad)
        bx = _tensor(boxes).to(device=device, dtype=dtype).clone().requires_grad_(want_grad)
    device = x.device
    gtc = _tensor(gt_cls).to(device=device, dtype=torch.int64)
    gtn = normalise_gt(_tensor(gt_boxes).to(device), frame, dtype)
    B, Q, n1 = x.shape
    C, M = n1 - 1, gtn.shape[1]
    present = (gtc >= 0) & (gtc < C)
    out = {}
    with torch.no_grad():
        p = torch.softmax(x, dim=-1)                                              # [B,Q,C+1]
        pc = torch.gather(p, 2, gtc.clamp(0, C - 1)[:, None, :].expand(B, Q, M)).permute(0, 2, 1)   # [B,M,Q]
        l1 = (bx[:, None, :, :] - gtn[:, :, None, :]).abs().sum(-1)               # [B,M,Q]
        gi = giou(xyxy(bx)[:, None, :, :], xyxy(gtn)[:, :, None, :])
        cost = (-costs[0] * pc + costs[1] * l1 + -costs[2] * gi) * present[:, :, None]
        cost_np = cost.double().cpu().numpy()
        frozen = None if match is None else np.asarray(_tensor(match).cpu().numpy(), np.int64).reshape(B, M)
        match = np.full((B, M), -1, np.int32)
        tgt = np.full((B, Q), -1, np.int32)
        gap, excess = math.inf, math.inf
        for b in range(B if frozen is not None else 0):
            for m in range(M):
                if frozen[b, m] >= 0:
                    match[b, m] = frozen[b, m]
                    tgt[b, frozen[b, m]] = m
        for b in range(B if frozen is None else 0):
            rows = [m for m in range(M) if present[b, m]]
            r2c, total_cost = (solver or solve_assignment)(cost_np[b], rows)
            for m in rows:
                match[b, m] = r2c[m]
                tgt[b, r2c[m]] = m
            if want_gap and rows:
                gap = min(gap, match_gap(cost_np[b], rows, r2c, total_cost))
                excess = min(excess, greedy_cost(cost_np[b], rows) - total_cost)
        out.update(cost=cost, gap_match=gap, greedy_excess=excess)
    bi, mi = np.nonzero(match >= 0)
    qi = match[bi, mi]
    bi_t, mi_t, qi_t = (torch.as_tensor(v, dtype=torch.int64, device=device) for v in (bi, mi, qi))
    t = torch.full((B, Q), C, dtype=torch.int64, device=device)
    t[bi_t, qi_t] = gtc[bi_t, mi_t]
    wt = torch.ones(C + 1, dtype=dtype, device=device)
    wt[C] = eos
    ce = torch.nn.functional.cross_entropy(x.reshape(-1, n1), t.reshape(-1), weight=wt)       # sum wt * nll / sum wt
    n = max(len(bi), 1)
    if len(bi):
        pb, pg = bx[bi_t, qi_t], gtn[bi_t, mi_t]
        l1_l = (pb - pg).abs().sum() / n
        gi_l = (1.0 - giou(xyxy(pb), xyxy(pg))).sum() / n
    else:
        l1_l = gi_l = bx.sum() * 0.0
    total = w[0] * ce + w[1] * l1_l + w[2] * gi_l
    out.update(match=torch.as_tensor(match), tgt=torch.as_tensor(tgt), loss=torch.stack([ce, l1_l, gi_l, total]).detach(),
               total=total)
    if want_grad and not attached:
        gl, gb = torch.autograd.grad(total, (x, bx), allow_unused=True)
        out["grad_logits"] = gl.detach()
        out["grad_boxes"] = torch.zeros_like(bx) if gb is None else gb.detach()
    return out


def oracle_postprocess(logits, boxes, frame=FRAME, thr=CONF_THR, max_det=None):
    """detr_detector.py:186-202 restated in float32 torch for a batch, kept queries in query order
    -> (dets [B,max_det,6], counts [B,2], gap_score, gap_lead)."""
    x, bx = _tensor(logits).float(), _tensor(boxes).float()
    B, Q, _ = x.shape
    max_det = Q if max_det is None else max_det
    W, H = frame
    dets = np.zeros((B, max_det, 6), np.float32)
    counts = np.zeros((B, 2), np.int32)
    probs = x.softmax(-1)[..., :-1]
    scores, labels = probs.max(-1)
    p64 = _tensor(logits).double().softmax(-1)[..., :-1]
    top = torch.topk(p64, min(2, p64.shape[-1]), dim=-1).values
    gap_lead = ((top[..., 0] - top[..., 1]) / top[..., 0]).min().item() if top.shape[-1] > 1 else math.inf
    gap_score = (top[..., 0] - float(np.float32(thr))).abs().min().item()
    for b in range(B):
        keep = scores[b] > thr
        cx, cy, w, h = bx[b][keep].unbind(-1)
        rows = torch.stack([(cx - 0.5 * w) * W, (cy - 0.5 * h) * H, (cx + 0.5 * w) * W, (cy + 0.5 * h) * H, scores[b][keep],
                            labels[b][keep].float()], dim=-1).numpy()
        k = min(len(rows), max_det)
        dets[b, :k] = rows[:k]
        counts[b] = (k, len(rows))
    return dets, counts, gap_score, gap_lead


def score_tol(C: int) -> float:
    """How far two float32 evaluations of a query's score may lie apart.  One evaluation of p = exp(x - max) / sum: the sum of
    n = C + 1 non-negative terms added in any order is within (n - 1) u of the exact sum (u = 2^-24, relative); the exps of
    numerator and denominator are within 2 ulp = 4 u each, the subtraction and the division within u each: (C + 10) u in
    all, absolute as well since p <= 1.  Two evaluations (the kernel or the host build against torch's float32 softmax) are
    within twice that -- a tenth of the 1e-4 the scores keep from the threshold for C = 91."""
    return 2 * (C + 10) * 2.0 ** -24


def exact_score_expectations(post):
    """post(logits, boxes, thr, max_det) -> (dets, counts) as numpy arrays: the output stage on setdet_cases.score_inputs and
    at max_det = 1, max_det = 1024 with Q = 65, all and none of 65 queries kept.  Shared by the host and the device test."""
    x, bx = score_inputs()
    with np.errstate(invalid="ignore"):
        e = np.exp(x[0] - np.nanmax(x[0], axis=1, keepdims=True))
        p = (e / e.sum(1, keepdims=True, dtype=np.float32))[:, :2]
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert p[0].tolist() == [0.5, 0.5] and p[3].tolist() == [0.0, 0.0] and p[4, 0] == p[4, 1] and np.isnan(p[2]).all()
    W, H = FRAME
    for thr, rows in ((0.5, []), (below, [0]), (0.0, [0, 1, 4])):         # the comparison is strict: 0.5 > 0.5 keeps nothing
        dets, counts = post(x, bx, thr, None)
        assert counts.tolist() == [[len(rows), len(rows)]], (thr, counts)
        assert (dets[0, len(rows):] == 0).all()
        for k, q in enumerate(rows):
            cx, cy, w, h = bx[0, q]
            assert dets[0, k, :4].tolist() == [(cx - 0.5 * w) * W, (cy - 0.5 * h) * H, (cx + 0.5 * w) * W, (cy + 0.5 * h) * H]
            assert dets[0, k, 5] == np.argmax(p[q]) == (0, 1, None, None, 0)[q]       # numpy: the first maximum
            assert abs(dets[0, k, 4] - p[q].max()) <= score_tol(2)
        if rows:
            assert dets[0, 0, 4] == 0.5                                    # exp(0) / (1 + 1 + 0): exact in any order
    # max_det = 1 on `limits`: the first kept query alone
    c = BY_ID["limits"]
    ref = reference(c)
    want, wcounts, _, _ = ref["post"]
    dets, counts = post(ref["logits"], ref["boxes"], CONF_THR, 1)
    assert dets.shape == (1, 1, 6) and counts.tolist() == [[1, int(wcounts[0, 1])]] and wcounts[0, 1] > 1
    assert np.array_equal(dets[0, 0, :4], want[0, 0, :4]) and dets[0, 0, 5] == want[0, 0, 5]
    assert abs(dets[0, 0, 4] - want[0, 0, 4]) <= score_tol(c.C)
    # Q = 65, one live lane in the output stage's second wave: max_det = 1024 leaves zero rows past the kept ones; every
    # query kept (conf_thr = -1); none kept (conf_thr = 1)
    c = BY_ID["q65-n65"]
    ref = reference(c)
    want, wcounts, _, _ = ref["post"]
    dets, counts = post(ref["logits"], ref["boxes"], CONF_THR, 1024)
    assert dets.shape == (c.B, 1024, 6) and np.array_equal(counts, wcounts)
    for b in range(c.B):
        k = int(wcounts[b, 0])
        assert np.array_equal(dets[b, :k, :4], want[b, :k, :4]) and np.array_equal(dets[b, :k, 5], want[b, :k, 5])
        assert (dets[b, k:] == 0).all()
    every = oracle_postprocess(ref["logits"], ref["boxes"], thr=-1.0)
    dets, counts = post(ref["logits"], ref["boxes"], -1.0, None)
    assert (counts == 65).all() and np.array_equal(counts, every[1])
    assert np.array_equal(dets[..., :4], every[0][..., :4]) and np.array_equal(dets[..., 5], every[0][..., 5])
    assert np.abs(dets[..., 4] - every[0][..., 4]).max() <= score_tol(c.C)
    dets, counts = post(ref["logits"], ref["boxes"], 1.0, None)
    assert (counts == 0).all() and (dets == 0).all()


# ---- the host build -------------------------------------------------------------------------------------------------------
class CSpec(ctypes.Structure):   # GsrSetDetSpec of include/gsraster.h
    _fields_ = [("B", ctypes.c_int32), ("Q", ctypes.c_int32), ("C", ctypes.c_int32), ("M", ctypes.c_int32),
                ("img_w", ctypes.c_float), ("img_h", ctypes.c_float), ("c_class", ctypes.c_float), ("c_l1", ctypes.c_float),
                ("c_giou", ctypes.c_float), ("w_ce", ctypes.c_float), ("w_l1", ctypes.c_float), ("w_giou", ctypes.c_float),
                ("eos_coef", ctypes.c_float), ("conf_thr", ctypes.c_float), ("max_det", ctypes.c_int32), ("flags", ctypes.c_uint32)]


def c_spec(B, Q, C, M, frame=FRAME, costs=(C_CLASS, C_L1, C_GIOU), w=(W_CE, W_L1, W_GIOU), eos=EOS, thr=CONF_THR, max_det=None):
    return CSpec(B, Q, C, M, frame[0], frame[1], costs[0], costs[1], costs[2], w[0], w[1], w[2], eos, thr,
                 Q if max_det is None else max_det, 0)


def host_sources():
    return os.path.join(HM, "setdet_host.cpp"), [os.path.join(CSRC, n) for n in ("gsr_setdet.h", "gsr_detmath.h", "gsr_math.h")]


def host_lib():
    lib = host_build.host_lib("setdet")
    vp = ctypes.c_void_p
    for fn in (lib.sdh_run_f32, lib.sdh_run_f64):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(CSpec), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    lib.sdh_post_f32.restype = ctypes.c_int
    lib.sdh_post_f32.argtypes = [ctypes.POINTER(CSpec), vp, vp, vp, vp]
    return lib


def host_run(lib, logits, boxes, gt_boxes, gt_cls, double=False, want_grad=True, frozen=None, **kw):
    """-> dict(match int32 [B,M], tgt int32 [B,Q], cost [B,M,Q], loss[4], grad_logits, grad_boxes or None) as numpy arrays of
    the precision asked for.  frozen = (match, tgt) of an earlier run: the match is taken from there instead of being
    computed (what the contract's gradient holds constant)."""
    ft = np.float64 if double else np.float32
    x = np.ascontiguousarray(logits, dtype=ft)
    bx = np.ascontiguousarray(boxes, dtype=ft)
    gtb = np.ascontiguousarray(gt_boxes, dtype=ft)
    gtc = np.ascontiguousarray(gt_cls, dtype=np.int32)
    B, Q, n1 = x.shape
    M = gtb.shape[1]
    cs = c_spec(B, Q, n1 - 1, M, **kw)
    loss = np.full((4,), np.nan, ft)
    gl = np.full(x.shape, np.nan, ft) if want_grad else None
    gb = np.full(bx.shape, np.nan, ft) if want_grad else None
    match = np.full((B, M), -9, np.int32) if frozen is None else np.ascontiguousarray(frozen[0], dtype=np.int32).copy()
    tgt = np.full((B, Q), -9, np.int32) if frozen is None else np.ascontiguousarray(frozen[1], dtype=np.int32).copy()
    cost = np.full((B, M, Q), np.nan, ft)
    fn = lib.sdh_run_f64 if double else lib.sdh_run_f32
    rc = fn(ctypes.byref(cs), x.ctypes.data, bx.ctypes.data, gtb.ctypes.data, gtc.ctypes.data, loss.ctypes.data,
            gl.ctypes.data if want_grad else None, gb.ctypes.data if want_grad else None, match.ctypes.data, tgt.ctypes.data,
            cost.ctypes.data, 0 if frozen is None else 1)
    assert rc == 0
    return dict(match=match, tgt=tgt, cost=cost, loss=loss, grad_logits=gl, grad_boxes=gb)


def host_post(lib, logits, boxes, thr=CONF_THR, max_det=None, frame=FRAME):
    x = np.ascontiguousarray(logits, dtype=np.float32)
    bx = np.ascontiguousarray(boxes, dtype=np.float32)
    B, Q, n1 = x.shape
    cs = c_spec(B, Q, n1 - 1, 1, frame=frame, thr=thr, max_det=max_det)
    dets = np.full((B, cs.max_det, 6), np.nan, np.float32)
    counts = np.full((B, 2), -9, np.int32)
    assert lib.sdh_post_f32(ctypes.byref(cs), x.ctypes.data, bx.ctypes.data, dets.ctypes.data, counts.ctypes.data) == 0
    return dets, counts


# ---- a reference computed once per case and shared by the tests that need it -----------------------------------------------
_CACHE = {}


def reference(c: Case):
    """-> dict(logits, boxes, gt_boxes, gt_cls (numpy, read-only), o64: the float64 oracle's output, yard: {tensor: the
    float32 oracle's err}, yard_match_equal, post: oracle_postprocess's output)."""
    if c.id not in _CACHE:
        logits, boxes, gtb, gtc = make_inputs(c)
        for a in (logits, boxes, gtb, gtc):
            a.setflags(write=False)
        o64 = oracle(logits, boxes, gtb, gtc, torch.float64, want_gap=True)
        o32 = oracle(logits, boxes, gtb, gtc, torch.float32)
        yard = {k: err(o32[k], o64[k]) for k in COMPARED}
        _CACHE[c.id] = dict(logits=logits, boxes=boxes, gt_boxes=gtb, gt_cls=gtc, o64=o64, yard=yard,
                            yard_match_equal=bool(torch.equal(o32["match"], o64["match"]) and torch.equal(o32["tgt"], o64["tgt"])),
                            yard_cost_err=float((o32["cost"].double() - o64["cost"]).abs().max()),
                            post=oracle_postprocess(logits, boxes))
    return _CACHE[c.id]


def check_with_match_frozen(who, got, inputs, **kw):
    """loss, grad_logits and grad_boxes of got (dict, with its match [B,M]) against the float64 oracle run with got's match
    frozen; the yardstick is the float32 oracle with the same match.  Prints each figure, then asserts the usual bound."""
    m = np.asarray(_tensor(got["match"]).cpu().numpy())
    o64 = oracle(*inputs, torch.float64, match=m, **kw)
    o32 = oracle(*inputs, torch.float32, match=m, **kw)
    fails = []
    for k in COMPARED:
        e, y = err(got[k], o64[k]), err(o32[k], o64[k])
        print(f"{who} {k}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {bound(y):.3e}")
        if not e <= bound(y):
            fails.append((k, e, bound(y)))
    assert not fails, f"{who}: {fails}"
    return o64


def tie_reference(kind):
    """-> dict(inputs, cost: the float64 oracle's cost matrix [M,Q], optimum: its optimum's cost summed exactly, match: its
    match, gap: the smallest distance between distinct values of one row of cost), computed once."""
    key = "tie:" + kind
    if key not in _CACHE:
        inputs = tie_inputs(kind)
        for a in inputs:
            a.setflags(write=False)
        o = oracle(*inputs, torch.float64, want_grad=False)
        cost = o["cost"][0].numpy()
        match = o["match"][0].numpy()
        _CACHE[key] = dict(inputs=inputs, cost=cost, match=match, optimum=assignment_cost(cost, match),
                           gap=min(distinct_gap(r) for r in cost))
    return _CACHE[key]


def check_tie(who, kind, got, want_match):
    """got (dict of match [1,M], tgt [1,Q], loss, grad_logits, grad_boxes) on tie_inputs(kind): match integer-equal to
    want_match (the host build's, what the stated rule gives), one-to-one with tgt its inverse, as cheap as the oracle's
    optimum in the oracle's own float64 cost matrix to 1e-12 relative (equal pairs have the same double there, so only the
    order of the sum can differ), and loss and gradients within the bound of the oracle with this match frozen."""
    ref = tie_reference(kind)
    match = np.asarray(_tensor(got["match"]).cpu().numpy()).reshape(-1)
    tgt = np.asarray(_tensor(got["tgt"]).cpu().numpy()).reshape(-1)
    assert match.tolist() == np.asarray(want_match).reshape(-1).tolist(), f"{who} {kind}: match {match.tolist()}"
    assert match.min() >= 0 and match.max() < TIE_Q and len(set(match.tolist())) == TIE_M
    want_tgt = np.full(TIE_Q, -1, np.int32)
    want_tgt[match] = np.arange(TIE_M)
    assert np.array_equal(tgt, want_tgt), f"{who} {kind}: tgt is not the inverse of match"
    total = assignment_cost(ref["cost"], match)
    print(f"{who} {kind}: match {match.tolist()} costs {total!r}, the oracle's optimum {ref['optimum']!r}")
    assert abs(total - ref["optimum"]) <= 1e-12 * abs(ref["optimum"])
    check_with_match_frozen(f"{who} {kind}", got, ref["inputs"])


def margins_ok(ref) -> bool:
    return ref["o64"]["gap_match"] > GAP_MATCH and ref["post"][2] > GAP_SCORE and ref["post"][3] > GAP_LEAD


def covers(c: Case, ref) -> bool:
    """What the case claims to exercise (test_the_cases_cover_what_they_claim spells it out)."""
    o = ref["o64"]
    kept = ref["post"][1][:, 1]
    claim = EDGE_CLAIMS.get(c.id.split("#")[0])                       # (the seed search appends #seed to the id)
    if claim is not None:
        present = (ref["gt_cls"] >= 0) & (ref["gt_cls"] < c.C)
        ok = (c.B * c.Q) % 4 == claim["bq_mod4"] and c.B > claim.get("images_above", 0)
        ok = ok and term_blocks(c) > claim.get("term_blocks_above", 0)
        ok = ok and bool(present.all()) and bool((o["match"].numpy() >= 0).all())            # every present row matched
        # the output stage keeps a query and drops a query somewhere in the batch (per image it cannot hold for Q = 3)
        return ok and (c.Q == 1 or bool((kept > 0).any() and (kept < c.Q).any()))
    if c.kind == "contested":
        return o["greedy_excess"] > GAP_MATCH
    if c.kind in ("plain", "ragged") and c.Q > 1:
        return bool((kept > 0).all() and (kept < c.Q).all())
    return True


if __name__ == "__main__":
    # the seed search: for every case the first seed that meets the margin conditions and what the case claims
    lib = host_lib()
    for c in CASES:
        own = reference(c)                                                        # the committed seed holds what it must
        assert margins_ok(own) and covers(c, own) and own["yard_match_equal"], f"{c.id}: seed {c.seed} does not hold"
        for seed in range(300):
            t = c._replace(seed=seed, id=f"{c.id}#{seed}")
            ref = reference(t)
            if margins_ok(ref) and covers(t, ref) and ref["yard_match_equal"]:
                o = ref["o64"]
                h = host_run(lib, ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"])
                ratios = {k: (err(h[k], o[k]), ref["yard"][k]) for k in COMPARED}
                print(f"{c.id}: seed={seed} gap_match={o['gap_match']:.2e} greedy_excess={o['greedy_excess']:.2e} "
                      f"gap_score={ref['post'][2]:.2e} gap_lead={ref['post'][3]:.2e} kept={ref['post'][1][:, 1].tolist()} "
                      f"cost32={ref['yard_cost_err']:.2e} match_equal={np.array_equal(h['match'], o['match'].numpy())}")
                print("    host err / yardstick err: " + ", ".join(f"{k} {a:.2e}/{b:.2e}" for k, (a, b) in ratios.items()))
                break
        else:
            print(f"{c.id}: no seed found")

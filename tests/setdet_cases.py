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
python tests/setdet_cases.py searches the seeds.
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
]
BY_ID = {c.id: c for c in CASES}


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
           w=(W_CE, W_L1, W_GIOU), eos=EOS, want_grad=True, device="cpu", want_gap=False, solver=None):
    """The contract of include/gsraster.h in torch.  logits / boxes may be tensors that require grad (then `total` is
    returned attached and no backward is run here).  -> dict(match, tgt, cost, loss[4], total, grad_logits, grad_boxes,
    gap_match, greedy_excess).  solver (default solve_assignment): what matches one image's rows on the host."""
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
        match = np.full((B, M), -1, np.int32)
        tgt = np.full((B, Q), -1, np.int32)
        gap, excess = math.inf, math.inf
        for b in range(B):
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


def margins_ok(ref) -> bool:
    return ref["o64"]["gap_match"] > GAP_MATCH and ref["post"][2] > GAP_SCORE and ref["post"][3] > GAP_LEAD


def covers(c: Case, ref) -> bool:
    """What the case claims to exercise (test_the_cases_cover_what_they_claim spells it out)."""
    o = ref["o64"]
    kept = ref["post"][1][:, 1]
    if c.kind == "contested":
        return o["greedy_excess"] > GAP_MATCH
    if c.kind in ("plain", "ragged") and c.Q > 1:
        return bool((kept > 0).all() and (kept < c.Q).all())
    return True


if __name__ == "__main__":
    # the seed search: for every case the first seed that meets the margin conditions and what the case claims
    lib = host_lib()
    for c in CASES:
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

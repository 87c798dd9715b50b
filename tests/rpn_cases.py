"""Shared by the RPN proposal stage's tests (not a test module): the cases, an oracle written from the formulas of
include/gsraster.h (GsrRpnSpec) -- not from the kernels -- and the host build of csrc/gsr_rpn.h.

Two kinds of case.

EXACT: integer-valued cell anchors, all deltas 0, an integer frame, iou_thr 0.5 or 0.75.  With deltas 0 the decode is exact
(exp(0) = 1), every box is integer-valued, every area, intersection and union is an integer below 2^24, and with a union of
at most 2 * 10^6 the float32 quotient compares with 0.5 or 0.75 exactly as 2p > q or 4p > 3q does (the quotient of two such
integers is never within float32 rounding of 1/2 or 3/4 without being equal to it).  The oracle decides in integers; there
is no margin and nothing is left out.

FLOAT: Detectron2's real anchors, random deltas, iou_thr 0.7, at most 300 candidates.  The oracle computes in float64 and
asserts its own margins before anything is compared: every consulted |iou - thr|, every w - min_size and h - min_size of a
candidate with a finite box, and every gap between unequal logits exceed GAP = 1e-4, far above float32 decode error at these
magnitudes (coordinates below 2^10: an ulp is 6e-5 at most, a few ulps of error in a box side move an IoU by about 1e-6).
The seeds are fixed so that the margins hold; nothing is masked.  Decoded boxes may differ from the float64 oracle by
detloss_cases.bound(the float32 oracle's own error), as in the other stages' tests.
"""
import ctypes
import math
from functools import lru_cache
from typing import NamedTuple, Tuple

import numpy as np

import detloss_cases as DL
import host_build

bound, err = DL.bound, DL.err
GAP = 1e-4
DW_MAX = math.log(1000.0 / 16.0)
MAX_SLOTS, MAX_POST = 16384, 4096
SIZES, RATIOS = (32, 64, 128, 256, 512), (0.5, 1.0, 2.0)


# ---- anchors ---------------------------------------------------------------------------------------------------------------
def real_cell_anchors() -> np.ndarray:
    """Detectron2's generate_cell_anchors for SIZES x RATIOS, restated: doubles, then float32."""
    rows = []
    for s in SIZES:
        for r in RATIOS:
            w = math.sqrt(float(s) ** 2.0 / r)
            h = r * w
            rows.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    return np.array(rows, np.float32)


def int_cell_anchors(sizes=SIZES, ratios=RATIOS) -> np.ndarray:
    """The same shapes with even integer sides, so that the corners are integers."""
    rows = []
    for s in sizes:
        for r in ratios:
            w = 2 * round(s / math.sqrt(r) / 2.0)
            h = 2 * round(s * math.sqrt(r) / 2.0)
            rows.append([-w // 2, -h // 2, w // 2, h // 2])
    return np.array(rows, np.float32)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def flat_logits(logits_b: np.ndarray) -> np.ndarray:
    """[A,Hf,Wf] -> the logits in candidate-index order, i = (y * Wf + x) * A + a."""
    return np.ascontiguousarray(logits_b.transpose(1, 2, 0)).reshape(-1)


def order_desc(values: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """ids sorted by (value descending by float comparison, id ascending); values holds no NaN."""
    return ids[np.lexsort((ids, -values.astype(np.float64)))]


def logit_gap(values: np.ndarray) -> float:
    """The smallest gap between unequal values (inf if there is none); infinities are apart from everything."""
    v = np.unique(values[np.isfinite(values)].astype(np.float64))
    return float(np.diff(v).min()) if v.size > 1 else math.inf


class Level(NamedTuple):
    logits: np.ndarray      # [B,A,Hf,Wf] float32
    deltas: np.ndarray      # [B,4A,Hf,Wf] float32
    cell: np.ndarray        # [A,4] float32
    stride: int
    shift0: float


def oracle_select(lv: Level, frame, min_size: float, pre_topk: int, dtype=np.float64):
    """-> dict(boxes [B,n,4] dtype, scores [B,n] float32, valid [B,n] bool, index [B,n] int32 (-1: unused rank),
    size_gap, logit_gap) for the n = min(pre_topk, A*Hf*Wf) ranks of this level."""
    B, A, Hf, Wf = lv.logits.shape
    n_in = A * Hf * Wf
    n = min(pre_topk, n_in)
    boxes, scores = np.zeros((B, n, 4), dtype), np.zeros((B, n), np.float32)
    valid, index = np.zeros((B, n), bool), np.full((B, n), -1, np.int32)
    size_gap, lgap = math.inf, math.inf
    lim = dtype(DW_MAX)
    for b in range(B):
        v = flat_logits(lv.logits[b])
        ids = np.nonzero(~np.isnan(v))[0]
        lgap = min(lgap, logit_gap(v[ids]))
        top = order_desc(v[ids], ids)[:n]
        k = top.size
        index[b, :k] = top
        a, p = top % A, top // A
        y, x = p // Wf, p % Wf
        sx = (x * lv.stride).astype(dtype) + dtype(lv.shift0)
        sy = (y * lv.stride).astype(dtype) + dtype(lv.shift0)
        cell = lv.cell.astype(dtype)[a]
        anc = np.stack([cell[:, 0] + sx, cell[:, 1] + sy, cell[:, 2] + sx, cell[:, 3] + sy], 1)
        d = np.stack([lv.deltas[b, 4 * a + c, y, x] for c in range(4)], 1).astype(dtype)
        with np.errstate(all="ignore"):
            w, h = anc[:, 2] - anc[:, 0], anc[:, 3] - anc[:, 1]
            cx, cy = anc[:, 0] + dtype(0.5) * w, anc[:, 1] + dtype(0.5) * h
            dw = np.where(d[:, 2] < lim, d[:, 2], np.where(np.isnan(d[:, 2]), d[:, 2], lim))
            dh = np.where(d[:, 3] < lim, d[:, 3], np.where(np.isnan(d[:, 3]), d[:, 3], lim))
            pcx, pcy = d[:, 0] * w + cx, d[:, 1] * h + cy
            pw, ph = np.exp(dw) * w, np.exp(dh) * h
            raw = np.stack([pcx - dtype(0.5) * pw, pcy - dtype(0.5) * ph, pcx + dtype(0.5) * pw, pcy + dtype(0.5) * ph], 1)
            finite = np.isfinite(raw).all(1)
            clipped = np.stack([np.clip(raw[:, 0], 0, frame[0]), np.clip(raw[:, 1], 0, frame[1]),
                                np.clip(raw[:, 2], 0, frame[0]), np.clip(raw[:, 3], 0, frame[1])], 1).astype(dtype)
            bw, bh = clipped[:, 2] - clipped[:, 0], clipped[:, 3] - clipped[:, 1]
            ok = finite & (bw > dtype(min_size)) & (bh > dtype(min_size))
        if finite.any():
            size_gap = min(size_gap, float(np.abs(bw[finite].astype(np.float64) - min_size).min()),
                           float(np.abs(bh[finite].astype(np.float64) - min_size).min()))
        boxes[b, :k][ok] = clipped[ok]
        scores[b, :k][ok] = v[top][ok]
        valid[b, :k] = ok
    return dict(boxes=boxes, scores=scores, valid=valid, index=index, size_gap=size_gap, logit_gap=lgap)


def walk_order(scores_b: np.ndarray, level_b: np.ndarray) -> np.ndarray:
    slots = np.nonzero((level_b >= 0) & ~np.isnan(scores_b))[0]
    return order_desc(scores_b[slots], slots)


def oracle_walk(boxes_b: np.ndarray, scores_b: np.ndarray, level_b: np.ndarray, thr: float, post: int, exact: bool):
    """One image -> (keep list of slots, walked: the candidates examined, n_order, iou_gap).  exact: integer boxes, the
    verdict 2p > q (thr 0.5) or 4p > 3q (thr 0.75); otherwise float64 IoUs and the smallest |iou - thr| consulted."""
    order = walk_order(scores_b, level_b)
    if exact:
        bx = np.rint(boxes_b).astype(np.int64)
        assert np.array_equal(bx.astype(boxes_b.dtype), boxes_b) and np.abs(bx).max(initial=0) < (1 << 24)
        assert thr in (0.5, 0.75)
        num, den = (2, 1) if thr == 0.5 else (4, 3)
    else:
        bx = boxes_b.astype(np.float64)
    area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
    kb, ka, kl = np.zeros((post, 4), bx.dtype), np.zeros(post, bx.dtype), np.zeros(post, np.int64)
    keep, walked, gap = [], 0, math.inf
    for s in order:
        nk = len(keep)
        if nk >= post:
            break
        walked += 1
        m = kl[:nk] == level_b[s]
        sup = False
        if m.any():
            K, b = kb[:nk][m], bx[s]
            iw = np.maximum(np.minimum(K[:, 2], b[2]) - np.maximum(K[:, 0], b[0]), 0)
            ih = np.maximum(np.minimum(K[:, 3], b[3]) - np.maximum(K[:, 1], b[1]), 0)
            p = iw * ih
            q = ka[:nk][m] + area[s] - p
            if exact:
                assert q.max() <= 2_000_000 and q.min() >= 0
                sup = bool((num * p > den * q).any())
            else:
                with np.errstate(all="ignore"):
                    iou = p / q
                fin = ~np.isnan(iou)
                if fin.any():
                    gap = min(gap, float(np.abs(iou[fin] - thr).min()))
                sup = bool((iou[fin] > thr).any())
        if not sup:
            kb[nk], ka[nk], kl[nk] = bx[s], area[s], level_b[s]
            keep.append(int(s))
    return keep, walked, int(order.size), gap


def oracle_nms(boxes: np.ndarray, scores: np.ndarray, level: np.ndarray, thr: float, post: int, exact: bool):
    """-> dict(keep [B,post] int32, counts [B], proposals [B,post,4] (boxes' dtype), scores [B,post] float32, walked [B],
    n_order [B], iou_gap)."""
    B = scores.shape[0]
    out = dict(keep=np.full((B, post), -1, np.int32), counts=np.zeros(B, np.int32), proposals=np.zeros((B, post, 4), boxes.dtype),
               scores=np.zeros((B, post), np.float32), walked=np.zeros(B, np.int64), n_order=np.zeros(B, np.int64), iou_gap=math.inf)
    for b in range(B):
        keep, walked, n_order, gap = oracle_walk(boxes[b], scores[b], level[b], thr, post, exact)
        k = len(keep)
        out["keep"][b, :k], out["counts"][b] = keep, k
        out["proposals"][b, :k], out["scores"][b, :k] = boxes[b][keep], scores[b][keep]
        out["walked"][b], out["n_order"][b], out["iou_gap"] = walked, n_order, min(out["iou_gap"], gap)
    return out


# ---- the NMS entry alone: exact cases on hand-made slots -------------------------------------------------------------------------
class NmsCase(NamedTuple):
    id: str
    N: int
    post: int
    thr: float
    gen: str
    seed: int = 0


def _random_slots(rs, N, frame, smin, smax, nscore):
    """Integer boxes with many repeats, scores quantised to nscore values with +0.0 and -0.0 among them, levels -1, 0, 1."""
    w, h = rs.randint(smin, smax + 1, N), rs.randint(smin, smax + 1, N)
    step = max(smin // 2, 1)
    x1 = rs.randint(0, (frame - smax) // step + 1, N) * step
    y1 = rs.randint(0, (frame - smax) // step + 1, N) * step
    boxes = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    q = rs.randint(-nscore // 2, nscore // 2 + 1, N)
    scores = (q / 4.0).astype(np.float32)
    scores[(q == 0) & (rs.rand(N) < 0.5)] = np.float32(-0.0)
    level = rs.choice(np.array([-1, 0, 0, 1, 1], np.int32), N)
    dup = rs.rand(N) < 0.1                                                  # identical boxes with identical scores
    src = rs.randint(0, N, N)
    boxes[dup], scores[dup] = boxes[src[dup]], scores[src[dup]]
    return boxes, scores, level.astype(np.int32)


def _grid_slots(rs, N, cell=10, side=8, cols=128):
    """N pairwise disjoint boxes: every one is kept."""
    i = rs.permutation(N)
    x1, y1 = (i % cols) * cell, (i // cols) * cell
    boxes = np.stack([x1, y1, x1 + side, y1 + side], 1).astype(np.float32)
    return boxes, rs.permutation(N).astype(np.float32), np.zeros(N, np.int32)


def _chain_slots():
    """a suppresses b; b would suppress c, a does not: c is kept.  Once inside one chunk, once with fillers in between so
    that a, b and c fall into three chunks, once with b and c in the chunk behind a's.  Then identical boxes with identical
    scores (the lower slot wins), and coincident boxes on two levels (both stay).  Fillers are disjoint from everything."""
    a, b, c = [0, 0, 100, 100], [20, 0, 120, 100], [50, 0, 150, 100]
    boxes, scores, level = [], [], []

    def put(box, dy, s, lv=0):
        boxes.append([box[0], box[1] + dy, box[2], box[3] + dy]); scores.append(s); level.append(lv)

    s = 1000.0
    for gap_ab, gap_bc in ((0, 0), (70, 70), (70, 0)):                       # fillers between a and b, b and c
        dy = 200 * len(boxes)
        put(a, dy, s); s -= 1
        for _ in range(gap_ab):
            put([2000 + 12 * len(boxes), 0, 2010 + 12 * len(boxes), 10], 0, s); s -= 1
        put(b, dy, s); s -= 1
        for _ in range(gap_bc):
            put([2000 + 12 * len(boxes), 0, 2010 + 12 * len(boxes), 10], 0, s); s -= 1
        put(c, dy, s); s -= 1
    marks = dict(chains=[i for i, bx in enumerate(boxes) if bx[2] - bx[0] == 100])
    twin0 = len(boxes)
    put([300, 0, 340, 40], 0, 5.0); put([300, 0, 340, 40], 0, 5.0)           # identical twice: slot twin0 stays, twin0 + 1 goes
    put([300, 100, 340, 140], 0, 4.0, 0); put([300, 100, 340, 140], 0, 4.0, 1)    # two levels: both stay
    boxes.append([0, 0, 0, 0]); scores.append(9999.0); level.append(-1)      # not a candidate, whatever its score
    marks.update(twin0=twin0)
    return np.array(boxes, np.float32), np.array(scores, np.float32), np.array(level, np.int32), marks


NMS_CASES = (
    NmsCase("n1", 1, 1, 0.5, "random"),
    NmsCase("n63-thr75", 63, 63, 0.75, "random", 1),
    NmsCase("n64", 64, 64, 0.5, "random", 2),
    NmsCase("n65-thr75", 65, 65, 0.75, "random", 3),
    NmsCase("n129", 129, 129, 0.5, "random", 4),
    NmsCase("n129-cap-midchunk", 129, 37, 0.75, "sparse", 5),
    NmsCase("n129-cap-second-chunk", 129, 70, 0.5, "grid", 6),
    NmsCase("chains", 0, 0, 0.5, "chains"),
    NmsCase("n4097-all-kept-cap4096", 4097, 4096, 0.5, "grid", 7),
    NmsCase("n16384", 16384, 4096, 0.75, "big", 8),
)
NMS_B = 2


@lru_cache(maxsize=None)
def nms_inputs(c: NmsCase):
    """-> (boxes [B,N,4], scores [B,N], level [B,N], thr, post)."""
    if c.gen == "chains":
        bx, sc, lv, _ = _chain_slots()
        flip = bx.copy(); flip[:, [0, 2]] = bx[:, [1, 3]]; flip[:, [1, 3]] = bx[:, [0, 2]]      # image 1: transposed
        return np.stack([bx, flip]), np.stack([sc, sc]), np.stack([lv, lv]), c.thr, bx.shape[0]
    per = []
    for b in range(NMS_B):
        rs = np.random.RandomState(1000 * c.seed + b + 17)
        if c.gen == "random":
            per.append(_random_slots(rs, c.N, 100, 20, 60, 9))
        elif c.gen == "sparse":
            per.append(_random_slots(rs, c.N, 400, 20, 40, 41))
        elif c.gen == "big":
            per.append(_random_slots(rs, c.N, 1400, 8, 24, 2001))
        else:
            per.append(_grid_slots(rs, c.N))
    return tuple(np.stack([p[k] for p in per]) for k in range(3)) + (c.thr, c.post)


@lru_cache(maxsize=None)
def nms_reference(c: NmsCase):
    bx, sc, lv, thr, post = nms_inputs(c)
    return oracle_nms(bx, sc, lv, thr, post, exact=True)


# ---- select + NMS --------------------------------------------------------------------------------------------------------------
class LevelShape(NamedTuple):
    A: int
    Hf: int
    Wf: int
    stride: int


class Case(NamedTuple):
    id: str
    exact: bool
    levels: Tuple[LevelShape, ...]
    frame: Tuple[float, float]      # img_w, img_h
    pre_topk: int
    post: int
    thr: float
    gen: str
    seed: int = 0
    min_size: float = 0.0
    B: int = 2


C4 = (LevelShape(15, 50, 68, 16),)
# image 1: a share of spatially uncorrelated score and a bonus for the three smallest anchors, whose neighbours overlap least:
# enough keeps to stop at 4096 with thr 0.5
C4_NOISE, C4_SMALL = 1.0, 0.5
CASES = (
    # n_in = 105 < pre_topk, not a multiple of 64
    Case("short-level", True, (LevelShape(3, 5, 7, 16),), (112.0, 80.0), 200, 105, 0.5, "quant", 1),
    # the 100th place inside a tie group; +0.0 and -0.0 among the logits; n_in = 429
    Case("tie-at-k", True, (LevelShape(3, 11, 13, 8),), (104.0, 88.0), 100, 100, 0.75, "quant", 2),
    Case("one-anchor", True, (LevelShape(1, 1, 1, 32),), (64.0, 64.0), 5, 1, 0.5, "quant", 3),
    # one tie group of 67 500 > 2^16: every digit of the index decides
    Case("all-equal", True, (LevelShape(3, 150, 150, 4),), (600.0, 600.0), 300, 300, 0.5, "equal", 4),
    # 16 384 of 27 000
    Case("full-slots", True, (LevelShape(3, 100, 90, 8),), (720.0, 800.0), 16384, 4096, 0.5, "quant-fine", 5),
    # two levels chained; coincident anchors on the two levels
    Case("two-levels", True, (LevelShape(3, 11, 13, 8), LevelShape(3, 6, 7, 16)), (104.0, 88.0), 100, 150, 0.5, "quant", 6),
    # the C4 training shape: image 0 quantised blobs, image 1 all-distinct scores
    Case("c4-thr50-post4096", True, C4, (1088.0, 800.0), 12000, 4096, 0.5, "c4", 7),
    Case("c4-thr75-post2000", True, C4, (1088.0, 800.0), 12000, 2000, 0.75, "c4", 7),
    # float cases: Detectron2's anchors, random deltas, NaN and infinities
    Case("float-min0", False, (LevelShape(15, 4, 5, 64),), (320.0, 256.0), 280, 280, 0.7, "float", 12),
    Case("float-min16", False, (LevelShape(15, 3, 4, 64),), (256.0, 192.0), 1000, 180, 0.7, "float-outside", 12, 16.0),
    Case("float-two-levels", False, (LevelShape(15, 3, 3, 64), LevelShape(15, 2, 2, 128)), (256.0, 256.0), 120, 100, 0.7, "float", 13),
)
SMALL_INT_ANCHORS = np.array([[-8, -4, 8, 4], [-6, -6, 6, 6], [-4, -8, 4, 8]], np.float32) * 2


def _blobs(Hf, Wf, A, rs):
    y, x = np.mgrid[0:Hf, 0:Wf].astype(np.float64)
    f = np.zeros((Hf, Wf))
    for cy, cx, s in ((0.3, 0.25, 0.12), (0.6, 0.7, 0.18), (0.8, 0.3, 0.1)):
        f += np.exp(-(((y / Hf - cy) / s) ** 2 + ((x / Wf - cx) / s) ** 2))
    return f[None] * (1.0 + 0.15 * np.cos(np.arange(A))[:, None, None]) + 0.08 * rs.rand(A, Hf, Wf)


@lru_cache(maxsize=None)
def inputs(c: Case) -> Tuple[Level, ...]:
    rs = np.random.RandomState(c.seed)
    out = []
    for ls in c.levels:
        A, Hf, Wf = ls.A, ls.Hf, ls.Wf
        shape = (c.B, A, Hf, Wf)
        deltas = np.zeros((c.B, 4 * A, Hf, Wf), np.float32)
        if c.gen == "quant":
            q = rs.randint(-6, 7, shape)
            logits = (q / 2.0).astype(np.float32)
            logits[(q == 0) & (rs.rand(*shape) < 0.5)] = np.float32(-0.0)
        elif c.gen == "quant-fine":
            logits = (rs.randint(-3000, 3001, shape) / 8.0).astype(np.float32)
        elif c.gen == "equal":
            logits = np.full(shape, 1.5, np.float32)
        elif c.gen == "c4":
            img0 = np.round(_blobs(Hf, Wf, A, rs) * 150.0) / 16.0                       # a few hundred values
            cont = _blobs(Hf, Wf, A, rs) + C4_NOISE * rs.rand(A, Hf, Wf) + C4_SMALL * (np.arange(A) < 3)[:, None, None]
            img1 = np.empty(cont.size)
            img1[np.argsort(cont.reshape(-1), kind="stable")] = np.arange(cont.size) / 64.0 - 300.0    # all distinct
            logits = np.stack([img0, img1.reshape(A, Hf, Wf)]).astype(np.float32)
        else:                                                                # float, float-outside
            logits = (rs.randint(-40, 41, shape) / 8.0).astype(np.float32)
            deltas = (rs.randn(c.B, A, 4, Hf, Wf) * np.array([0.1, 0.1, 0.4, 0.4])[None, None, :, None, None]).astype(np.float32)
            deltas = deltas.reshape(c.B, 4 * A, Hf, Wf)
            flat_l, flat_d = logits.reshape(-1), deltas.reshape(c.B, A, 4, Hf * Wf)
            pick = rs.permutation(flat_l.size)
            flat_l[pick[0]], flat_l[pick[1]], flat_l[pick[2]], flat_l[pick[3]] = np.nan, np.inf, -np.inf, np.nan
            cells = rs.permutation(Hf * Wf)
            flat_d[0, 1, 2, cells[0]] = 5.0                                   # beyond the scale clamp
            flat_d[1, 2, 3, cells[1]] = 7.5
            flat_d[0, 3, 0, cells[0]] = np.nan
            flat_d[1, 4, 2, cells[1]] = np.inf                                # exp(inf) -> the clamp: the box stays finite
            flat_d[0, 5, 1, cells[2 % cells.size]] = -np.inf
            flat_d[1, 6, 0, cells[0]] = np.inf
            if c.gen == "float-outside":
                flat_d[0, 0, 0, cells[1]] = 40.0                              # wholly outside the frame, on either side
                flat_d[1, 1, 1, cells[2]] = -40.0
                flat_d[1, 7, 0, cells[0]] = 25.0
        if c.exact:
            cell = int_cell_anchors() if A == 15 else (SMALL_INT_ANCHORS[:A] if A == 3 else np.array([[-16, -16, 16, 16]], np.float32))
        else:
            cell = real_cell_anchors()
        out.append(Level(np.ascontiguousarray(logits), np.ascontiguousarray(deltas), cell, ls.stride, 0.0))
    return tuple(out)


def slots_of(c: Case):
    return [min(c.pre_topk, ls.A * ls.Hf * ls.Wf) for ls in c.levels]


@lru_cache(maxsize=None)
def reference(c: Case):
    """-> dict: cand_boxes (float64) / cand_boxes32 (the float32 oracle: the yardstick) / cand_scores / cand_level [B,N],
    index (per level, [B,n_l]), nms (oracle_nms on the float64 boxes), size_gap, logit_gap, iou_gap."""
    lvs, sizes = inputs(c), slots_of(c)
    N = sum(sizes)
    cb, cb32 = np.zeros((c.B, N, 4)), np.zeros((c.B, N, 4), np.float32)
    cs, cl = np.zeros((c.B, N), np.float32), np.full((c.B, N), -1, np.int32)
    index, size_gap, lgap, off = [], math.inf, math.inf, 0
    for l, (lv, n) in enumerate(zip(lvs, sizes)):
        o = oracle_select(lv, c.frame, c.min_size, c.pre_topk)
        o32 = oracle_select(lv, c.frame, c.min_size, c.pre_topk, np.float32)
        cb[:, off:off + n], cb32[:, off:off + n], cs[:, off:off + n] = o["boxes"], o32["boxes"], o["scores"]
        cl[:, off:off + n] = np.where(o["valid"], l, -1)
        index.append(o["index"])
        size_gap, lgap = min(size_gap, o["size_gap"]), min(lgap, o["logit_gap"])
        off += n
    nms = oracle_nms(cb, cs, cl, c.thr, c.post, c.exact)
    return dict(cand_boxes=cb, cand_boxes32=cb32, cand_scores=cs, cand_level=cl, index=index, nms=nms, size_gap=size_gap,
                logit_gap=lgap, iou_gap=nms["iou_gap"], N=N)


def proposals32(ref) -> np.ndarray:
    """The float32 oracle's boxes at the kept slots: the yardstick of the proposals."""
    n = ref["nms"]
    out = np.zeros(n["proposals"].shape, np.float32)
    for b in range(out.shape[0]):
        k = int(n["counts"][b])
        out[b, :k] = ref["cand_boxes32"][b][n["keep"][b, :k]]
    return out


def margins_ok(c: Case, ref) -> bool:
    """Exact cases need none; a float case's every gap exceeds GAP."""
    return c.exact or (ref["iou_gap"] > GAP and ref["size_gap"] > GAP and ref["logit_gap"] > GAP)


def box_check(who: str, got, ref64, ref32):
    """got within bound(the float32 oracle's error) of the float64 oracle; prints the figures first."""
    e, y = err(got, ref64), err(ref32, ref64)
    print(f"{who}: err {e:.3e} yardstick {y:.3e} bound {bound(y):.3e}")
    assert e <= bound(y), (who, e, y, bound(y))


# ---- the host build ----------------------------------------------------------------------------------------------------------
class CSpec(ctypes.Structure):   # GsrRpnSpec of include/gsraster.h
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("Hf", ctypes.c_int32), ("Wf", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("shift0", ctypes.c_float), ("img_w", ctypes.c_float), ("img_h", ctypes.c_float),
                ("min_size", ctypes.c_float), ("pre_topk", ctypes.c_int32), ("level", ctypes.c_int32),
                ("cand_offset", ctypes.c_int32), ("N", ctypes.c_int32), ("post_topk", ctypes.c_int32),
                ("iou_thr", ctypes.c_float), ("flags", ctypes.c_uint32)]


def c_spec(**kw) -> CSpec:
    s = CSpec()
    s.B = s.A = s.Hf = s.Wf = s.stride = s.pre_topk = s.N = s.post_topk = 1
    s.img_w = s.img_h = 1.0
    s.iou_thr = 0.5
    for k, v in kw.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    return s


def level_spec(c: Case, l: int, off: int, N: int) -> CSpec:
    ls, lv = c.levels[l], inputs(c)[l]
    return c_spec(B=c.B, A=ls.A, Hf=ls.Hf, Wf=ls.Wf, stride=ls.stride, shift0=lv.shift0, img_w=c.frame[0], img_h=c.frame[1],
                  min_size=c.min_size, pre_topk=c.pre_topk, level=l, cand_offset=off, N=N, post_topk=c.post, iou_thr=c.thr)


def host_lib():
    lib = host_build.host_lib("rpn")
    vp, sp = ctypes.c_void_p, ctypes.POINTER(CSpec)
    lib.ph_select.argtypes = [sp] + [vp] * 7
    lib.ph_nms.argtypes = [sp] + [vp] * 7
    lib.ph_select.restype = lib.ph_nms.restype = ctypes.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_nms(lib, boxes, scores, level, thr, post):
    B, N = scores.shape
    s = c_spec(B=B, N=N, post_topk=post, iou_thr=thr)
    out = dict(proposals=np.empty((B, post, 4), np.float32), scores=np.empty((B, post), np.float32), keep=np.empty((B, post), np.int32),
               counts=np.empty(B, np.int32))
    bx, sc, lv = (np.ascontiguousarray(a) for a in (boxes.astype(np.float32), scores, level))
    assert lib.ph_nms(ctypes.byref(s), _p(bx), _p(sc), _p(lv), _p(out["proposals"]), _p(out["scores"]), _p(out["keep"]),
                      _p(out["counts"])) == 0
    return out


@lru_cache(maxsize=None)
def host_propose(c: Case):
    """The host build over the case's levels, chained through cand_offset -> dict(cand_boxes, cand_scores, cand_level, index,
    nms)."""
    lib = host_lib()
    lvs, sizes = inputs(c), slots_of(c)
    N = sum(sizes)
    cb, cs, cl = np.full((c.B, N, 4), -1.0, np.float32), np.full((c.B, N), -1.0, np.float32), np.full((c.B, N), -7, np.int32)
    index, off = [], 0
    for l, (lv, n) in enumerate(zip(lvs, sizes)):
        idx = np.empty((c.B, n), np.int32)
        s = level_spec(c, l, off, N)
        assert lib.ph_select(ctypes.byref(s), _p(lv.logits), _p(lv.deltas), _p(lv.cell), _p(cb), _p(cs), _p(cl), _p(idx)) == 0
        index.append(idx)
        off += n
    return dict(cand_boxes=cb, cand_scores=cs, cand_level=cl, index=index, nms=host_nms(lib, cb, cs, cl, c.thr, c.post), N=N)

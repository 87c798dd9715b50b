"""Cases and oracle of the FPN RoI pooler (gsr_fpn_pool, gsr_fpn_pool_backward), shared by the CPU and the device tests.

Levels.  The oracle's level is the threshold form of include/gsraster.h in float64 on the float32 RoIs: q = sqrt(area) /
canonical_size + 1e-8, level = the number of thresholds q reaches; -1 beyond the count and for a non-finite row.  Every
live finite row of non-negative area is declared, and the helper asserts the declaration before anyone compares:
  EXACT   q equals a threshold (or is far from all of them) by construction: the sides are small integers or quarters, the
          area a perfect square of an integer, so float32 and float64 compute the same q and the comparison is exact
  NEAR    the three rows placed a hundredth of a pixel from a threshold on purpose (111.99 x 112, 112.01 x 112, 223.99 x
          224).  Their |q - thr| / thr is 4.5e-5, 4.5e-5 and 2.2e-5: under the 1e-4 asked of an undeclared row, and 70 x
          above what float32 can move q (two differences, a product, a root and a quotient, each within 2^-24 relative:
          under 3e-7 together).  They must keep |q - thr| / thr > 1e-5, 30 x that.
  (none)  |q - thr| / thr > 1e-4 for every threshold

Pooled values and gradients come from rcnn_cases.oracle_roi_align once per level, the rows of the other levels set to NaN
(which that oracle pools to zero), summed over the levels; float64 is the reference and the same code in float32 the
yardstick, compared through rcnn_cases' err / bound (4 x the yardstick's error, floor 2^-22, never above 1e-3).
"""
import ctypes
import math
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import torch

import host_build
import rcnn_cases as RC

bound, err, GAP = RC.bound, RC.err, RC.GAP
NEAR_GAP = 1e-5

STRIDES = (4, 8, 16, 32)
SIZES = ((97, 125), (49, 63), (25, 32), (13, 16))      # (Hf, Wf) per level: ragged 8 x 8 tiles on every one
NL = len(STRIDES)
CANON_SIZE, CANON_LEVEL = 224.0, 4
THR = (0.0,) + tuple(2.0 ** (int(math.log2(STRIDES[0])) + l - CANON_LEVEL) for l in range(1, NL))     # -, 0.5, 1, 2
P0 = 2                                                  # the first level is p2
B = 2
CFS = (3, 70)
POOL = ((7, 7, 0), (14, 14, 0), (3, 5, 2))
NAN, INF = float("nan"), float("inf")
X0, Y0 = 10.25, 20.5

EXACT, NEAR, FAR, NEG = "exact", "near", "far", "negative-area"
# (w, h, the level on the p2..p5 scale, how the row is declared)
TABLE = (
    (112.0, 112.0, 3, EXACT),       # exactly on the threshold
    (111.99, 112.0, 2, NEAR),
    (112.01, 112.0, 3, NEAR),
    (224.0, 224.0, 4, EXACT),
    (223.99, 224.0, 3, NEAR),
    (448.0, 448.0, 5, EXACT),
    (447.9, 448.0, 4, FAR),
    (98.0, 512.0, 4, EXACT),        # area exactly 224^2
    (49.0, 256.0, 3, EXACT),
    (196.0, 1024.0, 5, EXACT),
    (16.0, 784.0, 3, EXACT),
    (1.0, 1.0, 2, FAR),
    (3000.0, 3000.0, 5, FAR),       # the clamp
    (0.0, 0.0, 2, FAR),
    (-50.0, 60.0, 2, NEG),          # by definition
    (-300.0, -300.0, 4, FAR),       # positive area
)


def _box(w, h, x0=X0, y0=Y0):
    return [x0, y0, x0 + w, y0 + h]


# straddling the map's edges (the frame is 500 x 388): near corner, far corner, far edge of one axis; then an inverted RoI
# (x2 < x1: a negative area, level 0 by definition; its samples run backwards at a fixed ratio, its adaptive grid is 0)
EDGES = ([-30.5, -20.25, 60.75, 70.5], [430.5, 300.25, 560.0, 420.75], [200.25, 350.5, 330.5, 430.0], [200.4, 30.3, 120.2, 90.8])
EDGE_DECL = (FAR, FAR, FAR, NEG)
INVERTED = (0, len(TABLE) + 2 + 3)                      # (image, row) of the inverted RoI
_IMG0 = [_box(w, h) for w, h, _, _ in TABLE] + [[NAN, 10.0, 50.0, 60.0], [10.0, 20.0, INF, 60.0]] + [list(e) for e in EDGES] + \
    [_box(50.0, 50.0), _box(300.0, 300.0), [NAN] * 4]                               # the last three: beyond the count
_DECL0 = [d for _, _, _, d in TABLE] + [None, None] + list(EDGE_DECL)
# image 1: no level-5 RoI; its own mix, shifted origins
_IMG1 = [_box(30.5, 40.25, 100.5, 50.25), _box(112.0, 112.0, 200.0, 100.0), _box(224.0, 224.0, 150.0, 90.0), _box(60.25, 70.5, 300.0, 200.0),
         _box(150.5, 100.25, 20.0, 30.0), _box(300.25, 250.5, 90.0, 60.0), _box(8.5, 9.25, 400.0, 300.0), _box(100.0, 200.0, 350.0, 150.0),
         [NAN, NAN, NAN, NAN], _box(20.25, 300.5, 470.0, 60.0), _box(440.0, 30.5, 30.0, 340.0), _box(75.5, 75.5, 5.0, 5.0)]
_DECL1 = [FAR, EXACT, EXACT, FAR, FAR, FAR, FAR, FAR, None, FAR, FAR, FAR]
S = len(_IMG0)                                          # 24
_IMG1 = _IMG1 + [_box(448.0, 448.0)] * (S - len(_IMG1))  # beyond the count: a level-5 box that must not count
ROIS = np.array([_IMG0, _IMG1], np.float32)
DECL = (_DECL0, _DECL1)
N_ROI = np.array([[S - 3, 1], [12, 0]], np.int32)       # read with stride 2, like the sampler's counts
N_ROI_ZERO = np.array([[S - 3, 5], [0, 9]], np.int32)   # image 1: count 0
ROIS.setflags(write=False)
N_ROI.setflags(write=False)
N_ROI_ZERO.setflags(write=False)
EXPECT0 = tuple(p - P0 for _, _, p, _ in TABLE)         # the table's levels as indices


class Case(NamedTuple):
    Cf: int
    PH: int
    PW: int
    ratio: int

    @property
    def id(self):
        return f"c{self.Cf}-{self.PH}x{self.PW}-r{self.ratio}"


CASES = tuple(Case(cf, ph, pw, r) for cf in CFS for ph, pw, r in POOL)


# ---- levels -----------------------------------------------------------------------------------------------------------------
def _count(n_roi, stride, b, S_):
    return S_ if n_roi is None else min(max(int(np.asarray(n_roi).reshape(-1)[b * stride]), 0), S_)


def level_q(rois, dtype=np.float64):
    """[...,4] float32 rows -> q in `dtype` (NaN for a negative area)."""
    r = np.asarray(rois, np.float32).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        area = (r[..., 2] - r[..., 0]) * (r[..., 3] - r[..., 1])
        return np.sqrt(area) / dtype(CANON_SIZE) + dtype(1e-8)


def oracle_levels(rois, n_roi, stride, thr=THR, dtype=np.float64):
    """-> (roi_level int32 [B,S], level_list: per image and level the ascending rows, level_count int32 [B,nl])."""
    rois = np.asarray(rois, np.float32)
    Bn, S_ = rois.shape[:2]
    nl = len(thr)
    q = level_q(rois, dtype)
    with np.errstate(invalid="ignore"):
        lv = sum((q >= dtype(thr[l])).astype(np.int32) for l in range(1, nl)) if nl > 1 else np.zeros(q.shape, np.int32)
    lv = np.where(np.isfinite(rois).all(-1), lv, -1).astype(np.int32)
    for b in range(Bn):
        lv[b, _count(n_roi, stride, b, S_):] = -1
    lists = [[[s for s in range(S_) if lv[b, s] == l] for l in range(nl)] for b in range(Bn)]
    counts = np.array([[len(x) for x in row] for row in lists], np.int32)
    return lv, lists, counts


def check_declarations():
    """Every live finite row of the two images is declared and its declaration holds; the table's levels are the oracle's."""
    lv, _, _ = oracle_levels(ROIS, N_ROI, 2)
    q = level_q(ROIS)
    for b in range(B):
        for s in range(int(N_ROI[b, 0])):
            decl = DECL[b][s]
            if not np.isfinite(ROIS[b, s]).all():
                assert decl is None and lv[b, s] == -1, (b, s)
                continue
            assert decl is not None, f"row {(b, s)} is not declared"
            if decl == NEG:
                assert math.isnan(q[b, s]) and lv[b, s] == 0, (b, s)
                continue
            gap = min(abs(q[b, s] - t) / t for t in THR[1:])
            if decl == EXACT:
                r = ROIS[b, s].astype(np.float64)
                w, h = r[2] - r[0], r[3] - r[1]
                root = round(math.sqrt(w * h))
                assert w * 4 == int(w * 4) and h * 4 == int(h * 4) and root * root == w * h, (b, s)      # exact in float32 too
                assert level_q(ROIS[b, s], np.float32) == np.float32(q[b, s]), (b, s)
            elif decl == NEAR:
                assert NEAR_GAP < gap < GAP, (b, s, gap)
            else:
                assert gap > GAP, f"row {(b, s)}: |q - thr| / thr = {gap:.2e}"
    assert tuple(int(v) for v in lv[0, :len(TABLE)]) == EXPECT0
    assert (lv[0, S - 3:] == -1).all() and (lv[1, 12:] == -1).all() and lv[0, len(TABLE)] == lv[0, len(TABLE) + 1] == -1
    assert not (lv[1] == NL - 1).any() and all((lv[0] == l).any() for l in range(NL))
    return True


def detectron2_levels_f32(rois):
    """Detectron2's assign_boxes_to_levels in float32 torch: floor(canonical_level + log2(sqrt(area) / canonical_size + 1e-8)),
    clamped to the levels, as an index into them."""
    r = torch.tensor(np.array(rois, np.float32))
    sizes = torch.sqrt((r[..., 2] - r[..., 0]) * (r[..., 3] - r[..., 1]))
    lv = torch.floor(CANON_LEVEL + torch.log2(sizes / CANON_SIZE + 1e-8))
    return (torch.clamp(lv, min=P0, max=P0 + NL - 1).to(torch.int64) - P0).numpy()


# ---- pooled values and gradients ----------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(Cf: int, PH: int, PW: int):
    """-> (features: one read-only [B,Cf,Hf,Wf] per level, grad_pooled [B,S,Cf,PH,PW])."""
    rs = np.random.RandomState(311 + Cf)
    feats = tuple(rs.standard_normal((B, Cf, h, w)).astype(np.float32) for h, w in SIZES)
    gp = rs.standard_normal((B, S, Cf, PH, PW)).astype(np.float32)
    for a in feats + (gp,):
        a.setflags(write=False)
    return feats, gp


def masked_rois(rois, roi_level, l):
    """The rows of level l, every other row NaN: what the single-level entries pool to zero."""
    out = np.array(rois, np.float32)
    out[np.asarray(roi_level) != l] = NAN
    return out


def run(c: Case, dtype, n_roi=N_ROI):
    feats, gp = inputs(c.Cf, c.PH, c.PW)
    lv, _, _ = oracle_levels(ROIS, n_roi, 2)
    fs = [torch.tensor(f).to(dtype).requires_grad_(True) for f in feats]
    pooled, gap, grids = 0, math.inf, []
    for l, f in enumerate(fs):
        p, g, gp_l = RC.oracle_roi_align(f, masked_rois(ROIS, lv, l), n_roi, 2, c.PH, c.PW, 1.0 / STRIDES[l], c.ratio, dtype)
        pooled, gap = pooled + p, min(gap, gp_l)
        grids.append(g)
    (pooled * torch.tensor(gp).to(dtype)).sum().backward()
    out = dict(pooled=pooled.detach(), grids=np.stack(grids), gap=gap)
    for l, f in enumerate(fs):
        out[f"grad{l}"] = f.grad.detach() if f.grad is not None else torch.zeros_like(f.detach())
    return out


COMPARED = ("pooled",) + tuple(f"grad{l}" for l in range(NL))


@lru_cache(maxsize=None)
def reference(c: Case):
    assert check_declarations()
    o64, o32 = run(c, torch.float64), run(c, torch.float32)
    same_grid = bool((o64["grids"] == o32["grids"]).all())
    return dict(o64=o64, yard={k: err(o32[k], o64[k]) for k in COMPARED}, gap_grid=min(o64["gap"], o32["gap"]) if same_grid else 0.0)


def margins_ok(ref) -> bool:
    return ref["gap_grid"] > GAP


# ---- the host build -------------------------------------------------------------------------------------------------------
class CSpec(ctypes.Structure):   # GsrFpnSpec of include/gsraster.h
    _fields_ = [("B", ctypes.c_int32), ("S", ctypes.c_int32), ("Cf", ctypes.c_int32), ("PH", ctypes.c_int32), ("PW", ctypes.c_int32),
                ("sampling_ratio", ctypes.c_int32), ("nl", ctypes.c_int32), ("Hf", ctypes.c_int32 * 5), ("Wf", ctypes.c_int32 * 5),
                ("scale", ctypes.c_float * 5), ("thr", ctypes.c_float * 5), ("canonical_size", ctypes.c_float)]


def c_spec(Cf=1, PH=7, PW=7, ratio=0, S_=S, Bn=B, sizes=SIZES, strides=STRIDES, thr=THR) -> CSpec:
    s = CSpec(Bn, S_, Cf, PH, PW, ratio, len(sizes))
    for l, (h, w) in enumerate(sizes):
        s.Hf[l], s.Wf[l], s.scale[l], s.thr[l] = h, w, 1.0 / strides[l], thr[l]
    s.canonical_size = CANON_SIZE
    return s


def host_lib():
    lib = host_build.host_lib("fpn")
    vp, sp = ctypes.c_void_p, ctypes.POINTER(CSpec)
    lib.fh_assign.argtypes = [sp, vp, vp, ctypes.c_int32, vp, vp, vp]
    lib.fh_levels64.argtypes = [sp, vp, vp, ctypes.c_int32, vp]
    lib.fh_pool.argtypes = [sp, vp, vp, vp, vp]
    lib.fh_pool_bwd.argtypes = [sp, vp, vp, vp, vp]
    for fn in (lib.fh_assign, lib.fh_levels64, lib.fh_pool, lib.fh_pool_bwd):
        fn.restype = ctypes.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _pp(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


ISENT = -777


def host_assign(lib, rois=ROIS, n_roi=N_ROI, stride=2, spec=None):
    rois = np.ascontiguousarray(rois, np.float32)
    Bn, S_ = rois.shape[:2]
    s = spec if spec is not None else c_spec(S_=S_, Bn=Bn)
    n = None if n_roi is None else np.ascontiguousarray(n_roi)
    lv, lv64 = np.full((Bn, S_), ISENT, np.int32), np.full((Bn, S_), ISENT, np.int32)
    ll, lc = np.full((Bn, s.nl, S_), ISENT, np.int32), np.full((Bn, s.nl), ISENT, np.int32)
    assert lib.fh_assign(ctypes.byref(s), _p(rois), _p(n), stride, _p(lv), _p(ll), _p(lc)) == 0
    assert lib.fh_levels64(ctypes.byref(s), _p(rois), _p(n), stride, _p(lv64)) == 0
    return dict(roi_level=lv, level_list=ll, level_count=lc, roi_level64=lv64)


def host_pool(lib, c: Case, n_roi=N_ROI):
    feats, gp = inputs(c.Cf, c.PH, c.PW)
    feats = [np.ascontiguousarray(f) for f in feats]
    rois = np.ascontiguousarray(ROIS)
    s = c_spec(c.Cf, c.PH, c.PW, c.ratio)
    lv = host_assign(lib, n_roi=n_roi)["roi_level"]
    pooled = np.empty(gp.shape, np.float32)
    grads = [np.zeros(f.shape, np.float32) for f in feats]
    assert lib.fh_pool(ctypes.byref(s), _pp(feats), _p(rois), _p(lv), _p(pooled)) == 0
    assert lib.fh_pool_bwd(ctypes.byref(s), _p(rois), _p(lv), _p(np.ascontiguousarray(gp)), _pp(grads)) == 0
    out = dict(pooled=pooled)
    out.update({f"grad{l}": g for l, g in enumerate(grads)})
    return out


def edge_inputs():
    """rcnn_cases.roi_edge_inputs as a one-level pyramid of stride 1: the samples exactly at -1 and at n, and the next
    positions further out, through the pooler's own kernels -> (rcnn case, spec, (feat, grad_pooled, rois, n_roi), pooled
    [S,Cf] and grad [Cf,Hf,Wf] written out by hand)."""
    c, inputs, pooled, gf, _ = RC.roi_edge_inputs()
    rois = inputs[2]
    spec = c_spec(c.Cf, c.PH, c.PW, c.ratio, S_=rois.shape[1], Bn=1, sizes=((c.Hf, c.Wf),), strides=(1,), thr=(0.0,))
    return c, spec, inputs, pooled, gf


def host_pool_edges(lib):
    c, spec, (feat, gp, rois, n_roi), _, _ = edge_inputs()
    feat, gp, rois = (np.ascontiguousarray(a) for a in (feat, gp, rois))
    lv = host_assign(lib, rois=rois, n_roi=n_roi, spec=spec)["roi_level"]
    pooled, grad = np.empty(gp.shape, np.float32), np.zeros(feat.shape, np.float32)
    assert lib.fh_pool(ctypes.byref(spec), _pp([feat]), _p(rois), _p(lv), _p(pooled)) == 0
    assert lib.fh_pool_bwd(ctypes.byref(spec), _p(rois), _p(lv), _p(gp), _pp([grad])) == 0
    return pooled, grad


def lists_equal(level_list, level_count, lists) -> bool:
    """The live prefix of a [B,nl,S] list array equals the oracle's lists, and the counts their lengths."""
    ll, lc = np.asarray(level_list), np.asarray(level_count)
    return all(int(lc[b, l]) == len(rows) and ll[b, l, :len(rows)].tolist() == rows
               for b, per in enumerate(lists) for l, rows in enumerate(per))

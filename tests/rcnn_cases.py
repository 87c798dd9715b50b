"""Cases and oracle of the two-stage detector stage (gsr_rcnn_sample, gsr_roi_align, gsr_roi_align_backward, gsr_rcnn_loss,
gsr_rcnn_postprocess), shared by the CPU and the device tests.

The oracle is a PyTorch restatement of the formulas of include/gsraster.h with autograd for every gradient.  In float64
it is the reference; the same code in float32 on the CPU is the yardstick: a compared tensor (pooled, grad_features,
loss, grad_scores, grad_deltas) may be off by at most detloss_cases.bound(yardstick error) -- 4 x the yardstick's error
for that case and tensor, floor 2^-22, never above 1e-3.  Integer outputs must be integer-equal.

Decisions that a rounding could flip are kept away from their thresholds, and the oracle reports the distances:
  gap_fg    the smallest |best IoU - fg_iou| over the valid candidates                                   > 1e-4
  gap_lead  the smallest lead of the best row over the next one, over the candidates whose best IoU
            reaches fg_iou - 1e-4 (for a background candidate the row is not an output)                > 1e-4
  gap_grid  RoIAlign: the adaptive grid is the same integer in float32 and float64, and no sample lies
            within 1e-4 of -1 or of the map's far edge (where the read jumps to 0)                     > 1e-4
  gap_conf  the smallest |score - conf_thr|, and the lead of the best class over the next              > 1e-4
  gap_nms   the smallest |IoU - iou_thr| over pairs of candidates of one class                           > 1e-4

What the margins exclude is tested on inputs made by hand, whose expected outputs are literals here and equal in float32 and
float64: sample_exact_inputs (an IoU exactly at fg_iou, identical and absent gt rows), roi_edge_inputs (a sample exactly at -1
and at n, and the next positions further out), post_exact_inputs (a score exactly at conf_thr, a class tie),
post_poison_inputs (non-finite logits) and loss_guard_inputs (labels above C, gt_row outside 0 .. M - 1).  The cases past the
ones each stage was merged with sit where the kernels take another path than the scalar source (several items per thread,
a partial last block, a second turn of a strided loop, tiles that skip RoIs, maps with a side of 1); the CPU tests'
*_cases_cover_what_they_claim assert each premise from the oracle's outputs.
"""
import ctypes
import math
import os
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

import detloss_cases as DL
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
HM = os.path.join(ROOT, "tests", "host_math")

bound, err = DL.bound, DL.err
GAP = 1e-4
FRAME = (200.0, 160.0)          # img_w, img_h of the sampler, loss and output cases
BOX_W = (10.0, 10.0, 5.0, 5.0)
DW_MAX = math.log(1000.0 / 16.0)
M32 = 0xffffffff


# ---- the sampler ------------------------------------------------------------------------------------------------------------
def mix32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def sample_key(seed: int, b: int, i: int) -> int:
    return mix32((mix32((seed ^ ((b * 0x9E3779B9) & M32)) & M32) + i) & M32)


class SampleCase(NamedTuple):
    id: str
    R: int
    M: int
    S: int
    max_pos: int
    append_gt: bool = True
    n_prop: Optional[Tuple[int, int]] = None
    cls: Optional[Tuple[Tuple[int, ...], Tuple[int, ...]]] = None    # per image; default: every row present
    far: bool = False             # no proposal reaches fg_iou
    seed: int = 7
    data_seed: int = 0
    B: int = 2


NC = 5
B = 2
FG_IOU = 0.5

SAMPLE_CASES = (
    SampleCase("both-quotas", 6, 2, 4, 1),
    SampleCase("all-taken", 6, 2, 16, 16),
    SampleCase("past-a-wave", 70, 3, 32, 8),
    SampleCase("n1025", 1023, 2, 512, 128),
    SampleCase("n4096", 4064, 32, 1024, 256),
    SampleCase("n-prop", 70, 3, 32, 8, n_prop=(40, 0)),
    SampleCase("absent-rows", 70, 3, 32, 8, cls=((1, -1, NC), (-1, NC + 3, -5))),
    SampleCase("no-append", 70, 3, 32, 8, append_gt=False),
    SampleCase("gt-only-fg", 40, 1, 16, 4, far=True),
    SampleCase("gt-only-fg-no-append", 40, 1, 16, 4, append_gt=False, far=True),
    SampleCase("n1024", 1022, 2, 512, 128),                              # N = 1024 exactly: per = 1, every lane holds a candidate
    SampleCase("n3073", 3070, 3, 512, 128),                              # N = 3073: the first N with per = 4; both quotas bite
    SampleCase("n3072", 3069, 3, 512, 128),                              # N = 3072: per = 3 with every lane's three slots full
    SampleCase("n2049", 2047, 2, 512, 128),                              # N = 2049: the first N with per = 3; lanes from 683 on empty
)


def grid_boxes(rs, M):
    """M boxes in distinct cells of the frame: no two overlap."""
    cols = int(math.ceil(math.sqrt(M * FRAME[0] / FRAME[1])))
    rows = int(math.ceil(M / cols))
    cw, ch = FRAME[0] / cols, FRAME[1] / rows
    out = np.zeros((M, 4), np.float32)
    for m in range(M):
        cx0, cy0 = (m % cols) * cw, (m // cols) * ch
        w, h = cw * rs.uniform(0.55, 0.9), ch * rs.uniform(0.55, 0.9)
        x1, y1 = cx0 + rs.uniform(0.02, 0.08) * cw, cy0 + rs.uniform(0.02, 0.08) * ch
        out[m] = (x1, y1, x1 + w, y1 + h)
    return out


@lru_cache(maxsize=None)
def sample_inputs(c: SampleCase):
    """-> proposals [B,R,4], gt_boxes [B,M,4], gt_cls [B,M], n_prop [B] or None: read-only numpy arrays."""
    rs = np.random.RandomState(1000 + c.data_seed + c.R * 7 + c.M)
    gt = np.stack([grid_boxes(rs, c.M) for _ in range(c.B)])
    cls = np.array(c.cls, np.int32) if c.cls is not None else rs.randint(0, NC, size=(c.B, c.M)).astype(np.int32)
    prop = np.zeros((c.B, c.R, 4), np.float32)
    for b in range(c.B):
        g64 = torch.tensor(gt[b]).double()
        for i in range(c.R):
            while True:                                                # drawn again while its best IoU is within 1e-3 of fg_iou
                if not c.far and rs.uniform() < 0.4:
                    g = gt[b, rs.randint(c.M)]
                    w, h = g[2] - g[0], g[3] - g[1]
                    j = rs.uniform(-0.3, 0.3, 4) * np.array([w, h, w, h])
                    prop[b, i] = g + j
                else:
                    w, h = rs.uniform(4, 20 if c.far else 90), rs.uniform(4, 20 if c.far else 70)
                    x1, y1 = rs.uniform(0, FRAME[0] - w), rs.uniform(0, FRAME[1] - h)
                    prop[b, i] = (x1, y1, x1 + w, y1 + h)
                if abs(float(pair_iou(torch.tensor(prop[b, i:i + 1]).double(), g64).max()) - FG_IOU) > 1e-3:
                    break
    n_prop = None if c.n_prop is None else np.array(c.n_prop, np.int32)
    for a in (prop, gt, cls):
        a.setflags(write=False)
    return prop, gt, cls, n_prop


def pair_iou(a, g):
    """a [N,4], g [M,4] -> [N,M], Detectron2's pairwise_iou."""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = (torch.minimum(a[:, None, 2], g[None, :, 2]) - torch.maximum(a[:, None, 0], g[None, :, 0])).clamp(min=0)
    ih = (torch.minimum(a[:, None, 3], g[None, :, 3]) - torch.maximum(a[:, None, 1], g[None, :, 1])).clamp(min=0)
    inter = iw * ih
    return torch.where(inter > 0, inter / ((area_a[:, None] + area_g[None, :]) - inter), torch.zeros_like(inter))


def oracle_sample(prop, gt, cls, n_prop, C, S, max_pos, append_gt, seed, fg_iou=FG_IOU, dtype=torch.float64):
    """-> dict(idx, labels, gt_row int32 [B,S], rois float32 [B,S,4], counts int32 [B,2], gap_fg, gap_lead, keys, kinds)."""
    prop_t, gt_t = torch.as_tensor(np.array(prop)).to(dtype), torch.as_tensor(np.array(gt)).to(dtype)
    Bn, R, M = prop_t.shape[0], prop_t.shape[1], gt_t.shape[1]
    idx = np.full((Bn, S), -1, np.int32)
    labels, gt_row = np.full((Bn, S), -1, np.int32), np.full((Bn, S), -1, np.int32)
    rois, counts = np.zeros((Bn, S, 4), np.float32), np.zeros((Bn, 2), np.int32)
    gap_fg, gap_lead, keys, kinds = math.inf, math.inf, [], []
    for b in range(Bn):
        present = [0 <= int(cls[b, m]) < C for m in range(M)]
        npb = R if n_prop is None else min(max(int(n_prop[b]), 0), R)
        cand = torch.cat([prop_t[b], gt_t[b]]) if append_gt else prop_t[b]
        N = cand.shape[0]
        valid = [(i < npb) if i < R else present[i - R] for i in range(N)]
        iou = pair_iou(cand, gt_t[b])
        kind, row = [None] * N, [-1] * N            # None: not a candidate; True: foreground
        rows = [m for m in range(M) if present[m]]
        for i in range(N):
            if not valid[i]:
                continue
            kind[i] = False
            if not rows:
                continue
            v = iou[i, rows]
            best, k = v.max(0)
            best, m = float(best), rows[int((v == best).nonzero()[0])]
            gap_fg = min(gap_fg, abs(best - fg_iou))
            if best >= fg_iou - GAP and len(rows) > 1:
                gap_lead = min(gap_lead, best - float(torch.cat([v[:rows.index(m)], v[rows.index(m) + 1:]]).max()))
            if best >= fg_iou:
                kind[i], row[i] = True, m
        key = [sample_key(seed, b, i) for i in range(N)]
        fg = [i for i in range(N) if kind[i] is True]
        bg = [i for i in range(N) if kind[i] is False]
        n_pos = min(len(fg), max_pos)
        n_neg = min(len(bg), S - n_pos)
        taken = sorted(sorted(fg, key=lambda i: (key[i], i))[:n_pos] + sorted(bg, key=lambda i: (key[i], i))[:n_neg])
        for p, i in enumerate(taken):
            idx[b, p] = i
            rois[b, p] = (prop[b, i] if i < R else gt[b, i - R])
            labels[b, p] = int(cls[b, row[i]]) if kind[i] else C
            gt_row[b, p] = row[i] if kind[i] else -1
        counts[b] = (len(taken), n_pos)
        keys.append(key)
        kinds.append(kind)
    return dict(idx=idx, rois=rois, labels=labels, gt_row=gt_row, counts=counts, gap_fg=gap_fg, gap_lead=gap_lead, keys=keys,
                kinds=kinds)


def sample_margins_ok(o) -> bool:
    return o["gap_fg"] > GAP and o["gap_lead"] > GAP


@lru_cache(maxsize=None)
def sample_reference(c: SampleCase, seed: Optional[int] = None):
    prop, gt, cls, n_prop = sample_inputs(c)
    return oracle_sample(prop, gt, cls, n_prop, NC, c.S, c.max_pos, c.append_gt, c.seed if seed is None else seed)


def sample_exact_inputs():
    """The two exact decisions of match_candidate, which the margins keep the seeded cases away from -> (a SampleCase, its
    inputs, the expected idx / labels / gt_row / counts written out by hand).

    Every image has three copies of one gt box G = (10, 10, 20, 20), area 100.  Image 0: row 0 is absent (class -1), rows 1 and
    2 present (classes 2 and 3); image 1: classes (4, -1, 0).  The proposals:
      0  (10, 10, 20, 15), area 50 inside G: inter 50, union (50 + 100) - 50 = 100, IoU 50 / 100 = 0.5 in every precision;
         with fg_iou = 0.5 it is foreground (>=)
      1  G itself: IoU 1 with all three rows -- the first present one wins (row 1 in image 0, skipping the absent row 0 in
         front of it; row 0 in image 1)
      2  (10, 10, 20, 14): IoU 0.4, background
      3  (100, 100, 110, 110): IoU 0, background
    and the appended gt rows (candidates 4..6): the absent one is no candidate, the present ones match the first present row.
    S = 8 and max_pos = 8: everything is taken, in candidate order."""
    c = SampleCase("exact", 4, 3, 8, 8)
    G = (10.0, 10.0, 20.0, 20.0)
    prop = np.array([[(10.0, 10.0, 20.0, 15.0), G, (10.0, 10.0, 20.0, 14.0), (100.0, 100.0, 110.0, 110.0)]] * 2, np.float32)
    gt = np.array([[G, G, G]] * 2, np.float32)
    cls = np.array([[-1, 2, 3], [4, -1, 0]], np.int32)
    want = dict(idx=np.array([[0, 1, 2, 3, 5, 6, -1, -1], [0, 1, 2, 3, 4, 6, -1, -1]], np.int32),
                labels=np.array([[2, 2, NC, NC, 2, 2, -1, -1], [4, 4, NC, NC, 4, 4, -1, -1]], np.int32),
                gt_row=np.array([[1, 1, -1, -1, 1, 1, -1, -1], [0, 0, -1, -1, 0, 0, -1, -1]], np.int32),
                counts=np.array([[6, 4], [6, 4]], np.int32))
    return c, (prop, gt, cls, None), want


# ---- RoIAlign -----------------------------------------------------------------------------------------------------------------
HF, WF, SCALE = 9, 11, 1.0 / 16.0


class RoiCase(NamedTuple):
    Cf: int
    PH: int
    PW: int
    ratio: int
    Hf: int = HF
    Wf: int = WF
    scale: float = SCALE
    table: str = "base"           # base: ROIS / N_ROI below; wide, wide-zero, gen, prop: roi_table()
    name: Optional[str] = None
    S: int = 8                    # rows per image of a generated table
    seed: int = 0                 # of a generated table

    @property
    def id(self):
        return self.name or f"c{self.Cf}-{self.PH}x{self.PW}-r{self.ratio}"


WIDE = dict(Hf=9, Wf=27)          # 2 x 4 tiles of the backward: tiles_x != tiles_y
ROI_CASES = tuple(RoiCase(cf, ph, pw, r) for cf in (3, 70) for ph, pw in ((2, 2), (7, 7), (14, 14), (3, 5)) for r in (0, 2)) + \
    tuple(RoiCase(cf, 7, 7, r, table="wide", name=f"wide-c{cf}-r{r}", **WIDE) for cf in (1, 32, 33) for r in (0, 1, 16)) + (
    RoiCase(3, 7, 7, 2, table="wide", name="wide-c3-r2", **WIDE),            # the inverted rows' samples run backwards
    RoiCase(33, 7, 7, 0, table="wide-zero", name="wide-zero-c33-r0", **WIDE),  # image 1 has count 0
    RoiCase(3, 7, 7, 2, table="wide-zero", name="wide-zero-c3-r2", **WIDE),
    RoiCase(3, 3, 5, 0, Hf=1, Wf=11, table="gen", name="h1-r0"),
    RoiCase(3, 3, 5, 2, Hf=1, Wf=11, table="gen", name="h1-r2"),
    RoiCase(3, 3, 5, 0, Hf=9, Wf=1, table="gen", name="w1-r0"),
    RoiCase(3, 3, 5, 2, Hf=9, Wf=1, table="gen", name="w1-r2"),
    RoiCase(3, 2, 2, 0, Hf=1, Wf=1, table="gen", name="one-r0"),
    RoiCase(3, 2, 2, 2, Hf=1, Wf=1, table="gen", name="one-r2"),
    RoiCase(3, 7, 7, 0, Hf=8, Wf=16, table="gen", name="mult8-r0"),          # both sides exact multiples of the tile
    RoiCase(3, 7, 7, 2, Hf=8, Wf=16, table="gen", name="mult8-r2"),
    RoiCase(3, 7, 7, 0, Hf=16, Wf=24, scale=1.0, table="gen", name="scale-1"),
    RoiCase(3, 7, 7, 0, Hf=16, Wf=24, scale=0.25, table="gen", name="scale-quarter"),
    RoiCase(3, 14, 1, 0, table="gen", name="14x1-r0"),
    RoiCase(3, 1, 14, 2, table="gen", name="1x14-r2"),
    RoiCase(3, 2, 2, 0, table="prop", name="s1024", S=1024),                 # counts (1000, 0)
)
NAN = float("nan")
ROIS = np.array([
    [[20.3, 31.7, 101.9, 110.2],        # inside the map
     [-41.3, -29.2, 50.7, 61.1],        # across the near edge: samples below -1
     [101.3, 88.9, 203.1, 171.6],       # across the far edge: the y_low >= Hf - 1 branch and samples beyond the map
     [50.5, 50.5, 50.5, 50.5],          # zero area: grid 0 when adaptive
     [33.1, 35.2, 44.3, 46.9],          # inside one cell: many bins per pixel
     [0.4, 0.3, 175.7, 143.8],          # the whole map: an adaptive grid above 1
     [-4001.3, 10.2, 4203.4, 100.3],    # longer than 16 * PW cells: the cap
     [NAN, 10.0, 50.0, 60.0],           # a NaN row
     [60.2, 20.4, 130.8, 95.1],
     [10.9, 70.3, 90.2, 130.6]],
    [[5.2, 8.1, 60.3, 70.9],
     [120.4, 100.2, 170.3, 140.7],
     [70.1, 40.2, 75.3, 44.9],
     [30.3, 20.2, 160.4, 120.8],
     [0.2, 0.7, 20.1, 30.3],
     [88.8, 12.3, 140.1, 60.6],
     [15.5, 90.4, 60.6, 139.9],
     [20.0, 20.0, 100.0, 100.0],        # beyond n_roi from here on
     [NAN, NAN, NAN, NAN],
     [1.0e30, 0.0, 3.0e38, 50.0]]], np.float32)
N_ROI = np.array([[10, 1], [7, 0]], np.int32)      # read with stride 2, like the sampler's counts
ROIS.setflags(write=False)
N_ROI.setflags(write=False)


@lru_cache(maxsize=None)
def roi_inputs(Cf: int, PH: int, PW: int):
    rs = np.random.RandomState(77 + Cf)
    feat = rs.standard_normal((B, Cf, HF, WF)).astype(np.float32)
    gp = rs.standard_normal((B, ROIS.shape[1], Cf, PH, PW)).astype(np.float32)
    feat.setflags(write=False)
    gp.setflags(write=False)
    return feat, gp


# The wide map's table (9 x 27 cells at scale 1/16; a sample at feature position f comes from pixel (f + 0.5) * 16).  The
# backward's tiles start at x0 = 0, 8, 16, 24 and y0 = 0, 8; span_misses skips a RoI on an axis when its span [lo, hi]
# has hi < c0 - 2 or lo > c0 + 9.
ROIS_WIDE = np.array([
    [[28.3, 25.7, 91.9, 86.2],          # 0  x in cells 1..5:   the x0 = 0 tile alone
     [155.3, 30.2, 230.1, 90.7],        # 1  x in cells 9..14:  the x0 = 8 tile alone
     [283.1, 40.4, 355.6, 100.3],       # 2  x in cells 17..22: the x0 = 16 tile alone
     [401.3, 20.2, 425.7, 70.9],        # 3  the last column tile (x0 = 24, three columns wide)
     [60.2, 138.3, 100.4, 145.1],       # 4  y in (8.1, 8.6): the second row tile (y0 = 8, one row high) alone
     [120.0, 24.0, 232.0, 88.0],        # 5  x span [7, 14] exactly (bin 1): hi = 16 - 2, so `hi < c0 - 2` is false for x0 = 16 -- walked
     [152.0, 24.0, 264.0, 88.0],        # 6  x span [9, 16] exactly: lo = 0 + 9, so `lo > c0 + 9` is false for x0 = 0 -- walked
     [120.0, 24.0, 231.0, 88.0],        # 7  x span [7, 13.9375]: hi < 14, skipped by x0 = 16
     [153.0, 24.0, 264.0, 88.0],        # 8  x span [9.0625, 16]: lo > 9, skipped by x0 = 0
     [200.4, 30.3, 120.2, 90.8],        # 9  x inverted
     [300.2, 100.6, 380.9, 20.3],       # 10 y inverted
     [90.7, 120.2, 20.3, 40.9],         # 11 both inverted
     [400.2, 136.4, 420.3, 143.8]],     # 12 the far corner tile (x0 = 24, y0 = 8)
    [[390.3, 10.4, 430.2, 60.7],
     [10.2, 130.9, 50.6, 150.3],
     [140.7, 50.2, 250.3, 110.5],
     [260.3, 10.1, 270.9, 30.4],
     [330.3, 40.2, 280.1, 100.4],       # x inverted
     [20.0, 20.0, 100.0, 100.0],        # beyond n_roi from here on
     [NAN, NAN, NAN, NAN],
     [1.0e30, 0.0, 3.0e38, 50.0],
     [20.0, 20.0, 100.0, 100.0],
     [20.0, 20.0, 100.0, 100.0],
     [20.0, 20.0, 100.0, 100.0],
     [20.0, 20.0, 100.0, 100.0],
     [20.0, 20.0, 100.0, 100.0]]], np.float32)
N_ROI_WIDE = np.array([[13, 1], [5, 0]], np.int32)
N_ROI_WIDE_ZERO = np.array([[13, 3], [0, 9]], np.int32)       # image 1: count 0
WIDE_INVERTED = ((0, 9), (0, 10), (0, 11), (1, 4))
for _a in (ROIS_WIDE, N_ROI_WIDE, N_ROI_WIDE_ZERO):
    _a.setflags(write=False)
RB_TILE = 8


def span_misses(start, bin_, P, c0, dtype=np.float32):
    """csrc/gsr_rcnn.hip.h's span test restated, in `dtype`."""
    start, bin_ = dtype(start), dtype(bin_)
    end = dtype(start + dtype(dtype(P) * bin_))
    lo, hi = (start, end) if start < end else (end, start)
    return bool(hi < dtype(c0 - 2) or lo > dtype(c0 + RB_TILE + 1))


def roi_span(r, scale, PH, PW, dtype=np.float32):
    """-> (sy, by, sx, bx) of roi_axis, in `dtype`."""
    r, sc, half = np.asarray(r, np.float32).astype(dtype), dtype(np.float32(scale)), dtype(0.5)
    out = []
    for lo, hi, P in ((r[1], r[3], PH), (r[0], r[2], PW)):
        start = dtype(dtype(lo * sc) - half)
        end = dtype(dtype(hi * sc) - half)
        out += [start, dtype(dtype(end - start) / dtype(P))]
    return tuple(out)


def tiles_walked(c: "RoiCase", r, dtype=np.float32):
    """The tiles (y0, x0) of the backward that do not skip the finite RoI r."""
    sy, by, sx, bx = roi_span(r, c.scale, c.PH, c.PW, dtype)
    return [(y0, x0) for y0 in range(0, c.Hf, RB_TILE) for x0 in range(0, c.Wf, RB_TILE)
            if not span_misses(sy, by, c.PH, y0, dtype) and not span_misses(sx, bx, c.PW, x0, dtype)]


@lru_cache(maxsize=None)
def roi_table(c: RoiCase):
    """-> (rois float32 [B,S,4], n_roi int32 [B,2], read with stride 2), read-only."""
    if c.table == "base":
        return ROIS, N_ROI
    if c.table == "wide":
        return ROIS_WIDE, N_ROI_WIDE
    if c.table == "wide-zero":
        return ROIS_WIDE, N_ROI_WIDE_ZERO
    if c.table == "prop":                                             # drawn like the sampler's proposals, in the sampler's frame
        prop = sample_inputs(SampleCase("roi-prop", c.S, 3, 16, 4, data_seed=c.seed))[0]
        n_roi = np.array([[1000, 2], [0, 7]], np.int32)
        n_roi.setflags(write=False)
        return prop, n_roi
    assert c.table == "gen"
    # in feature cells: a near corner anywhere from two cells in front of the map to its far edge, a side from a fifth of a
    # cell to two cells more than the map's -- inside, across either edge, within one cell, over the whole map
    rs = np.random.RandomState(4000 + c.seed + 131 * c.Hf + 7 * c.Wf + c.PH)
    x1, y1 = rs.uniform(-2.0, c.Wf, (B, c.S)), rs.uniform(-2.0, c.Hf, (B, c.S))
    w, h = rs.uniform(0.2, c.Wf + 2.0, (B, c.S)), rs.uniform(0.2, c.Hf + 2.0, (B, c.S))
    sc = float(np.float32(c.scale))
    rois = (np.stack([x1 + 0.5, y1 + 0.5, x1 + w + 0.5, y1 + h + 0.5], -1) / sc).astype(np.float32)
    rois[0, 1] = [(-1.3 + 0.5) / sc, (-1.2 + 0.5) / sc, (c.Wf + 0.4 + 0.5) / sc, (c.Hf + 0.3 + 0.5) / sc]    # the whole map and beyond
    rois[1, c.S - 2] = NAN                                            # beyond n_roi
    rois[1, c.S - 1] = [1.0e30, 0.0, 3.0e38, 50.0]
    n_roi = np.array([[c.S, 1], [c.S - 2, 0]], np.int32)
    for a in (rois, n_roi):
        a.setflags(write=False)
    return rois, n_roi


@lru_cache(maxsize=None)
def roi_case_inputs(c: RoiCase):
    """-> (feat [B,Cf,Hf,Wf], grad_pooled [B,S,Cf,PH,PW], rois, n_roi); the base table on the base map: roi_inputs()."""
    rois, n_roi = roi_table(c)
    if c.table == "base" and (c.Hf, c.Wf) == (HF, WF):
        return roi_inputs(c.Cf, c.PH, c.PW) + (rois, n_roi)
    rs = np.random.RandomState(177 + c.Cf + 31 * c.Hf + c.Wf)
    feat = rs.standard_normal((B, c.Cf, c.Hf, c.Wf)).astype(np.float32)
    gp = rs.standard_normal((B, rois.shape[1], c.Cf, c.PH, c.PW)).astype(np.float32)
    feat.setflags(write=False)
    gp.setflags(write=False)
    return feat, gp, rois, n_roi


def roi_dead_rows(c: RoiCase):
    """The (b, s) whose pooled row must be zero whatever the features: beyond the count, or not finite."""
    rois, n_roi = roi_table(c)
    return [(b, s) for b in range(rois.shape[0]) for s in range(rois.shape[1])
            if s >= min(max(int(n_roi[b, 0]), 0), rois.shape[1]) or not np.isfinite(rois[b, s]).all()]


def _axis(lo, hi, scale, P, ratio, n, dtype):
    """One axis of one RoI -> (cell_lo [P,g], cell_hi, w_lo, w_hi, ok [P,g], grid, gap)."""
    start = lo * scale - 0.5
    end = hi * scale - 0.5
    length = end - start
    bin_ = length / P
    if ratio > 0:
        g = ratio
    else:
        cb = float(torch.ceil(bin_))
        g = 0 if math.isnan(cb) else int(min(max(cb, 0.0), 16.0))
    g = min(g, 16)
    if g == 0:
        return None, None, None, None, None, 0, math.inf
    p = torch.arange(P, dtype=dtype)[:, None]
    i = torch.arange(g, dtype=dtype)[None, :]
    y = start + p * bin_ + (i + 0.5) * bin_ / g
    ok = (y >= -1) & (y <= n)
    gap = float(torch.minimum((y + 1).abs(), (y - n).abs()).min())
    y = y.clamp(min=0)
    yl = y.floor().long().clamp(max=n - 1)
    top = yl >= n - 1
    yh = torch.where(top, yl, yl + 1).clamp(max=n - 1)
    y = torch.where(top, yl.to(dtype), y)
    ly = y - yl.to(dtype)
    return yl, yh, 1 - ly, ly, ok, g, gap


def oracle_roi_align(feat, rois, n_roi, stride, PH, PW, scale, ratio, dtype=torch.float64):
    """feat: a tensor [B,Cf,Hf,Wf] of `dtype` (it may require grad) -> (pooled [B,S,Cf,PH,PW], grids [B,S,2], gap)."""
    Bn, Cf, Hf, Wf = feat.shape
    r_all = torch.as_tensor(np.array(rois)).to(dtype)
    S = r_all.shape[1]
    sc = torch.tensor(scale, dtype=torch.float32).to(dtype)       # the float32 member, widened
    out, grids, gap = [], np.zeros((Bn, S, 2), np.int64), math.inf
    for b in range(Bn):
        n = S if n_roi is None else min(max(int(np.asarray(n_roi).reshape(-1)[b * stride]), 0), S)
        for s in range(S):
            r = r_all[b, s]
            zero = torch.zeros((Cf, PH, PW), dtype=dtype)
            if s >= n or not bool(torch.isfinite(r).all()):
                out.append(zero)
                continue
            yl, yh, hy, ly, oky, gy, g1 = _axis(r[1], r[3], sc, PH, ratio, Hf, dtype)
            xl, xh, hx, lx, okx, gx, g2 = _axis(r[0], r[2], sc, PW, ratio, Wf, dtype)
            grids[b, s] = (gy, gx)
            if gy == 0 or gx == 0:
                out.append(zero)
                continue
            gap = min(gap, g1, g2)
            f = feat[b]
            rows_l, rows_h = f[:, yl], f[:, yh]                    # [Cf,PH,gy,Wf]
            v1, v2, v3, v4 = rows_l[..., xl], rows_l[..., xh], rows_h[..., xl], rows_h[..., xh]      # [Cf,PH,gy,PW,gx]
            HY, LY = hy[None, :, :, None, None], ly[None, :, :, None, None]
            HX, LX = hx[None, None, None, :, :], lx[None, None, None, :, :]
            v = HY * HX * v1 + HY * LX * v2 + LY * HX * v3 + LY * LX * v4
            v = torch.where((oky[None, :, :, None, None] & okx[None, None, None, :, :]), v, torch.zeros_like(v))
            out.append(v.sum(dim=(2, 4)) / max(gy * gx, 1))
    return torch.stack(out).reshape(Bn, S, Cf, PH, PW), grids, gap


def roi_run(c: RoiCase, dtype):
    feat, gp, rois, n_roi = roi_case_inputs(c)
    f = torch.tensor(feat).to(dtype).requires_grad_(True)
    pooled, grids, gap = oracle_roi_align(f, rois, n_roi, 2, c.PH, c.PW, c.scale, c.ratio, dtype)
    (pooled * torch.tensor(gp).to(dtype)).sum().backward()
    return dict(pooled=pooled.detach(), grad_features=f.grad.detach(), grids=grids, gap=gap)


@lru_cache(maxsize=None)
def roi_reference(c: RoiCase):
    o64, o32 = roi_run(c, torch.float64), roi_run(c, torch.float32)
    yard = {k: err(o32[k], o64[k]) for k in ("pooled", "grad_features")}
    same_grid = bool((o64["grids"] == o32["grids"]).all())
    return dict(o64=o64, yard=yard, gap_grid=min(o64["gap"], o32["gap"]) if same_grid else 0.0)


def roi_margins_ok(ref) -> bool:
    return ref["gap_grid"] > GAP


def edge_pos(lo, hi, dtype):
    """The one sample of a 1-bin, ratio-1 axis at scale 1 (roi_axis and sample_pos of csrc/gsr_rcnn.h), rounded in `dtype`."""
    t = dtype
    lo, hi = t(np.float32(lo)), t(np.float32(hi))
    start, end = t(t(lo * t(1)) - t(0.5)), t(t(hi * t(1)) - t(0.5))
    bin_ = t(t(end - start) / t(1))
    return t(t(start + t(t(0) * bin_)) + t(t(t(0.5) * bin_) / t(1)))


def roi_edge_inputs():
    """The two exact edges of lerp_axis, which gap_grid keeps the seeded cases away from: one image, a 4 x 6 map of two
    channels holding distinct integers, scale 1, one bin, one sample per bin -> (case, (feat, grad_pooled, rois, n_roi),
    pooled [S,Cf] and grad_features [Cf,Hf,Wf] written out by hand, the per-row (y, x) cell or None).

    A RoI (lo, hi) puts its sample at (lo + hi) / 2 - 0.5.  (-3, 2) gives exactly -1: valid, clamped to cell 0 with weight 1.
    (2, 7) gives exactly 4 = Hf and (4, 9) exactly 6 = Wf: valid, the far border cell with weight 1.  Further out the read is 0:
    lo one float32 step below -3 (-1 - 2^-22 in float32, -1 - 2^-23 in float64) and 2^-21 below it, x's hi one float32 step
    above 9 (6 + 2^-21 in both) and y's hi two steps above 7 (4 + 2^-21 in both; one step gives 4 + 2^-22, which float32
    rounds back onto the edge, so that row would be decided by the rounding and is left out)."""
    Hf, Wf, Cf = 4, 6, 2
    c = RoiCase(Cf, 1, 1, 1, Hf=Hf, Wf=Wf, scale=1.0, name="edges")
    f32 = np.float32
    dn = lambda v: float(np.nextafter(f32(v), f32(-1e9)))
    up = lambda v: float(np.nextafter(f32(v), f32(1e9)))
    rows = [((-3.0, -3.0, 2.0, 2.0), (0, 0)),                              # the sample at (-1, -1)
            ((4.0, 2.0, 9.0, 7.0), (Hf - 1, Wf - 1)),                      # at (Hf, Wf)
            ((-3.0, 2.0, 2.0, 7.0), (Hf - 1, 0)),                          # at (Hf, -1)
            ((4.0, -3.0, 9.0, 2.0), (0, Wf - 1)),                          # at (-1, Wf)
            ((dn(-3.0), -3.0, 2.0, 2.0), None), ((-3.0, dn(-3.0), 2.0, 2.0), None),
            ((-3.0 - 2.0 ** -21, -3.0, 2.0, 2.0), None), ((-3.0, -3.0 - 2.0 ** -21, 2.0, 2.0), None),
            ((4.0, 2.0, up(9.0), 7.0), None), ((4.0, 2.0, 9.0, 7.0 + 2.0 ** -20), None)]
    rois = np.array([[r for r, _ in rows]], np.float32)
    S = len(rows)
    feat = (1.0 + np.arange(Cf * Hf * Wf, dtype=np.float32)).reshape(1, Cf, Hf, Wf)
    gp = (1.0 + np.arange(S * Cf, dtype=np.float32)).reshape(1, S, Cf, 1, 1)
    pooled, gf = np.zeros((S, Cf), np.float32), np.zeros((Cf, Hf, Wf), np.float32)
    for s, (_, cell) in enumerate(rows):
        if cell is not None:
            pooled[s] = feat[0, :, cell[0], cell[1]]
            gf[:, cell[0], cell[1]] += gp[0, s, :, 0, 0]                  # no cell is hit twice: each sum has one term
    return c, (feat, gp, rois, np.array([[S, 0]], np.int32)), pooled, gf, [cell for _, cell in rows]


# ---- the loss -------------------------------------------------------------------------------------------------------------------
class LossCase(NamedTuple):
    id: str
    C: int
    agnostic: bool = False
    beta: float = 0.0
    w: Tuple[float, float] = (1.0, 1.0)
    all_bg: bool = False          # no present row: every sampled row is background
    pad_image: bool = False       # image 1 holds padding rows only
    S: int = 16
    B: int = 2
    M: int = 2
    R: int = 30
    max_pos: int = 6
    spread: bool = False          # the gt rows' classes span 0 .. C - 1 (otherwise: the sampler cases' 0 .. 4, mod C)


LOSS_S, LOSS_R, LOSS_M = 16, 30, 2
LOSS_CASES = (
    LossCase("c1", 1),
    LossCase("c5-beta", 5, beta=0.5),
    LossCase("c80", 80),
    LossCase("c5-agnostic", 5, agnostic=True),
    LossCase("c80-agnostic-beta", 80, agnostic=True, beta=0.5),
    LossCase("c1-agnostic-beta", 1, agnostic=True, beta=0.5),
    LossCase("all-background", 5, all_bg=True),
    LossCase("padding-image", 5, pad_image=True, beta=0.5),
    LossCase("weights", 5, w=(0.7, 2.5)),
    LossCase("rows-33", 5, beta=0.5, B=3, S=11),                         # 33 rows: the last block holds one wave of four
    LossCase("s1024", 5, S=1024, R=1400, max_pos=1024),                  # 512 slab rows: two turns of slab_sum, eight of k_rcnn_count
    LossCase("c63", 63, M=6, max_pos=12, spread=True),
    LossCase("c64", 64, M=6, max_pos=12, spread=True, beta=0.5),
    LossCase("c65", 65, M=6, max_pos=12, spread=True),
    LossCase("c1024", 1024, M=6, max_pos=12, spread=True, beta=0.5),
    LossCase("c1024-agnostic", 1024, M=6, max_pos=12, spread=True, agnostic=True),
)
LOSS_COMPARED = ("loss", "grad_scores", "grad_deltas")


@lru_cache(maxsize=None)
def loss_inputs(c: LossCase):
    """-> dict of read-only numpy arrays: scores, deltas, rois, labels, gt_row, gt_boxes; zero_row: a (b, s) whose residual is
    exactly 0 (a ground-truth candidate: its target deltas are 0 in every precision, and so are its deltas), or None."""
    sc = SampleCase("loss", c.R, c.M, c.S, c.max_pos, data_seed=c.C, B=c.B)
    prop, gt, cls, _ = sample_inputs(sc)
    cls = np.array(cls) % c.C
    if c.spread:                                                       # 0 and C - 1 in every image, the rest evenly between
        cls = np.stack([np.roll(np.round(np.linspace(0, c.C - 1, c.M)).astype(np.int32), b) for b in range(c.B)])
    if c.all_bg:
        cls[:] = -1
    n_prop = np.array([c.R, 0], np.int32) if c.pad_image else None
    if c.pad_image:
        cls[1] = -1                                                    # no candidate at all in image 1
    smp = oracle_sample(prop, gt, cls, n_prop, c.C, c.S, c.max_pos, True, 11)
    assert sample_margins_ok(smp)
    rs = np.random.RandomState(500 + c.C)
    D = 4 if c.agnostic else 4 * c.C
    scores = (rs.standard_normal((c.B, c.S, c.C + 1)) * 2.0).astype(np.float32)
    deltas = (rs.standard_normal((c.B, c.S, D)) * 1.5).astype(np.float32)
    zero_row = None
    for b in range(c.B):
        for s in range(c.S):
            if smp["idx"][b, s] >= c.R and zero_row is None:           # a ground-truth candidate
                base = 0 if c.agnostic else 4 * int(smp["labels"][b, s])
                deltas[b, s, base:base + 4] = 0.0
                zero_row = (b, s)
    out = dict(scores=scores, deltas=deltas, rois=smp["rois"], labels=smp["labels"], gt_row=smp["gt_row"],
               gt_boxes=np.array(gt), counts=smp["counts"])
    for a in out.values():
        a.setflags(write=False)
    out["zero_row"] = zero_row
    return out


def oracle_loss(scores, deltas, rois, labels, gt_row, gt_boxes, agnostic=False, beta=0.0, w=(1.0, 1.0), box_w=BOX_W,
                dtype=torch.float64, want_grad=True):
    """-> dict(loss [3], grad_scores, grad_deltas)."""
    x = torch.tensor(np.array(scores)).to(dtype).requires_grad_(want_grad)
    d = torch.tensor(np.array(deltas)).to(dtype).requires_grad_(want_grad)
    r, gb = torch.tensor(np.array(rois)).to(dtype), torch.tensor(np.array(gt_boxes)).to(dtype)
    lb, gr = torch.tensor(np.array(labels)).long(), torch.tensor(np.array(gt_row)).long()
    Bn, S, n1 = x.shape
    C = n1 - 1
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    live = lb >= 0
    n = max(int(live.sum()), 1)
    logp = x - x.max(-1, keepdim=True).values
    logp = logp - logp.exp().sum(-1, keepdim=True).log()
    cls_term = -(logp.gather(-1, lb.clamp(min=0)[..., None])[..., 0] * live.to(dtype)).sum() / n
    fg = live & (lb < C) & (gr >= 0) & (gr < gb.shape[1])
    box_term = torch.zeros((), dtype=dtype)
    if bool(fg.any()):
        bi, si = fg.nonzero(as_tuple=True)
        src, dst = r[bi, si], gb[bi, gr[bi, si]]
        sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
        scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
        dw, dh = dst[:, 2] - dst[:, 0], dst[:, 3] - dst[:, 1]
        dcx, dcy = dst[:, 0] + 0.5 * dw, dst[:, 1] + 0.5 * dh
        t = torch.stack([f32(box_w[0]) * (dcx - scx) / sw, f32(box_w[1]) * (dcy - scy) / sh, f32(box_w[2]) * (dw / sw).log(),
                         f32(box_w[3]) * (dh / sh).log()], -1)
        base = torch.zeros_like(bi) if agnostic else 4 * lb[bi, si]
        pred = torch.stack([d[bi, si, base + k] for k in range(4)], -1)
        res = pred - t
        if beta > 0:
            bt = f32(beta)
            sl = torch.where(res.abs() < bt, 0.5 * res * res / bt, res.abs() - 0.5 * bt)
        else:
            sl = res.abs()
        box_term = sl.sum() / n
    total = f32(w[0]) * cls_term + f32(w[1]) * box_term
    out = dict(loss=torch.stack([cls_term, box_term, total]).detach())
    if want_grad:
        total.backward()
        out["grad_scores"] = x.grad.detach()
        out["grad_deltas"] = d.grad.detach() if d.grad is not None else torch.zeros_like(d.detach())     # no foreground row
    return out


@lru_cache(maxsize=None)
def loss_reference(c: LossCase):
    return loss_reference_of(c, loss_inputs(c))


def loss_reference_of(c: LossCase, i):
    args = (i["scores"], i["deltas"], i["rois"], i["labels"], i["gt_row"], i["gt_boxes"])
    o64 = oracle_loss(*args, agnostic=c.agnostic, beta=c.beta, w=c.w)
    o32 = oracle_loss(*args, agnostic=c.agnostic, beta=c.beta, w=c.w, dtype=torch.float32)
    return dict(o64=o64, yard={k: err(o32[k], o64[k]) for k in LOSS_COMPARED})


GUARD_CASE = "c5-beta"


@lru_cache(maxsize=None)
def loss_guard_inputs():
    """The guards of k_rcnn_rows and k_rcnn_count on the inputs of `c5-beta` -> (case, base, bad_labels, clean_labels,
    bad_rows, rows): bad_labels has C + 1, 2^31 - 1 and -7 on three live rows (one of them foreground) and clean_labels -1
    there -- the two must give the same bits; bad_rows has gt_row = M, M + 100 and -3 on three foreground rows (`rows`),
    which keep their cross-entropy term and gradient, add nothing to the box term and get a zero grad_deltas row."""
    c = next(k for k in LOSS_CASES if k.id == GUARD_CASE)
    base = loss_inputs(c)
    lb, gr = np.array(base["labels"]), np.array(base["gt_row"])
    fg = [(b, s) for b in range(c.B) for s in range(c.S) if 0 <= lb[b, s] < c.C and gr[b, s] >= 0 and (b, s) != base["zero_row"]]
    bg = [(b, s) for b in range(c.B) for s in range(c.S) if lb[b, s] == c.C]
    assert len(fg) >= 4 and len(bg) >= 2
    bad, clean = lb.copy(), lb.copy()
    for (b, s), v in zip((fg[0], bg[0], bg[1]), (c.C + 1, 2 ** 31 - 1, -7)):
        bad[b, s], clean[b, s] = v, -1
    rows = fg[1:4]
    bad_gr = gr.copy()
    for (b, s), v in zip(rows, (c.M, c.M + 100, -3)):
        bad_gr[b, s] = v
    return c, base, dict(base, labels=bad), dict(base, labels=clean), dict(base, gt_row=bad_gr), rows


# ---- the output stage ---------------------------------------------------------------------------------------------------------
class PostCase(NamedTuple):
    id: str
    conf: float
    max_det: int
    many: bool = False
    agnostic: bool = False
    R: int = 0                    # 0: the hand-made tables' 12 or 40; otherwise post_gen_inputs() places `ncand` candidates
    C: int = 3
    B: int = 2
    ncand: int = 0
    empty: Tuple[int, ...] = ()   # images with n_prop = 0


POST_C = 3
POST_CASES = (
    PostCase("conf-0.5", 0.5, 8),
    PostCase("conf-0.7", 0.7, 8),
    PostCase("agnostic-deltas", 0.5, 8, agnostic=True),
    PostCase("over-max-det", 0.5, 5, many=True),
    PostCase("r1024", 0.5, 250, R=1024, ncand=200),                      # per = 1, every thread holds a proposal
    PostCase("r1025", 0.5, 250, R=1025, ncand=200),                      # per = 2: the threads from 513 on hold none
    PostCase("r2049", 0.5, 300, R=2049, ncand=250),                      # per = 3
    PostCase("r4096", 0.5, 320, R=4096, ncand=400),                      # per = 4; k_rcnn_gather's loop beyond 256 rows
    PostCase("c64", 0.5, 20, R=70, C=64, ncand=30),
    PostCase("c1024", 0.5, 20, R=70, C=1024, ncand=30),
    PostCase("maxdet-1", 0.5, 1),
    PostCase("maxdet-R", 0.5, 40, many=True),
    PostCase("b3-empty-middle", 0.5, 20, R=70, B=3, ncand=30, empty=(1,)),
)
IOU_THR = 0.5


def _logits(C, cls, p, rs):
    """C + 1 logits whose softmax has p at `cls`, the rest spread unevenly."""
    rest = rs.uniform(0.5, 1.5, C + 1)
    rest[cls] = 0
    rest = rest / rest.sum() * (1 - p)
    rest[cls] = p
    return np.log(rest).astype(np.float32)


def post_gen_inputs(c: PostCase):
    """R proposals per image of which `ncand` are candidates (score 0.55 .. 0.95), at chosen indices: 0, 1023, 1024 and R - 1
    where the image has them, a run of eight in a row (every slot of two threads at four proposals per thread), the rest drawn
    over the whole range.  The candidates sit on disjoint sites of the frame; a quarter of the sites hold a second candidate
    shifted by a tenth of the box (IoU about 0.7), alternately of the same class (suppressed) and of another (kept).  Every
    other row has its best class at 0.3 .. 0.4 and the rest spread evenly.  The last image's n_prop is 37 short of R, with five
    rows behind it that would be candidates; an image of `empty` has n_prop = 0."""
    rs = np.random.RandomState(1700 + c.R + 3 * c.C + c.B)
    R, C, K, Bn = c.R, c.C, c.ncand, c.B
    D = 4 if c.agnostic else 4 * C
    deltas = (rs.standard_normal((Bn, R, D)) * 0.3).astype(np.float32)
    scores = np.zeros((Bn, R, C + 1), np.float32)
    prop = np.zeros((Bn, R, 4), np.float32)
    n_prop = np.full(Bn, R, np.int32)
    n_prop[Bn - 1] = R - 37
    for b in c.empty:
        n_prop[b] = 0
    for b in range(Bn):
        npb = int(n_prop[b]) if n_prop[b] > 0 else R                    # an empty image gets the same rows: they must not count
        w, h = rs.uniform(4, 40, R), rs.uniform(4, 40, R)
        x1, y1 = rs.uniform(0, FRAME[0] - w), rs.uniform(0, FRAME[1] - h)
        prop[b] = np.stack([x1, y1, x1 + w, y1 + h], -1)
        k0, p0 = rs.randint(C, size=R), rs.uniform(0.3, 0.4, R)
        scores[b] = np.log((1.0 - p0) / C)[:, None]
        scores[b, np.arange(R), k0] = np.log(p0)
        run0 = (npb // 2) // 8 * 8
        must = sorted({i for i in (0, 1023, 1024, R - 1) if i < npb} | set(range(run0, run0 + 8)))
        others = np.setdiff1d(np.arange(npb), must)
        cand = np.array(sorted(must + rs.choice(others, K - len(must), replace=False).tolist()))
        order = rs.permutation(K)                                        # candidate order[j] goes to site j (or is its twin)
        n_site = K - K // 4
        sites = grid_boxes(rs, n_site)
        site_cls = rs.randint(C, size=n_site)
        site_cls[:2] = (C - 1, 0)
        for j in range(K):
            i = int(cand[order[j]])
            site = j if j < n_site else j - n_site                       # the twins of the first K // 4 sites
            bx, k = sites[site].copy(), int(site_cls[site])
            if j >= n_site:
                bx[[0, 2]] += 0.1 * (bx[2] - bx[0])
                if site % 2 and C > 1:
                    k = (k + 1) % C
            prop[b, i] = bx
            scores[b, i] = _logits(C, k, float(rs.uniform(0.55, 0.95)), rs)
            o = 0 if c.agnostic else 4 * k
            deltas[b, i, o:o + 4] = (rs.uniform(-0.3, 0.3), rs.uniform(-0.3, 0.3), rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2))
        for i in range(npb, min(npb + 5, R)):                            # behind n_prop
            scores[b, i] = _logits(C, int(rs.randint(C)), 0.9, rs)
    for a in (scores, deltas, prop, n_prop):
        a.setflags(write=False)
    return scores, deltas, prop, n_prop


def post_candidates(c: PostCase):
    """The generator's premise, from the oracle's own candidate test: per image the ascending proposal indices above conf_thr."""
    scores, _, _, n_prop = post_inputs(c)
    p = torch.softmax(torch.tensor(np.array(scores)).double(), -1)[..., :c.C].max(-1).values.numpy()
    return [[i for i in range(int(n_prop[b])) if p[b, i] > float(np.float32(c.conf))] for b in range(c.B)]


@lru_cache(maxsize=None)
def post_inputs(c: PostCase):
    """-> scores [B,R,C+1], deltas [B,R,4C or 4], proposals [B,R,4], n_prop [B]."""
    if c.R:
        return post_gen_inputs(c)
    rs = np.random.RandomState(900 + int(c.conf * 10) + c.max_det)
    C = POST_C
    D = 4 if c.agnostic else 4 * C
    if c.many:
        R = 40
        prop = np.stack([grid_boxes(rs, R) for _ in range(B)])
        rows = [[(int(rs.randint(C)), float(rs.uniform(0.55, 0.95)), (0.1, -0.1, 0.05, 0.02)) for _ in range(R)] for _ in range(B)]
        rows[1] = [(k, 0.3, dl) for k, _, dl in rows[1]]               # image 1: no candidate
        n_prop = np.array([R, R], np.int32)
    else:
        R = 12
        base = np.array([40.0, 30.0, 100.0, 90.0], np.float32)
        other = np.array([120.0, 90.0, 180.0, 150.0], np.float32)
        prop = np.zeros((B, R, 4), np.float32)
        spec = [
            (base, 0, 0.90, (0.0, 0.0, 0.0, 0.0)),                     # two classes on one box: both kept
            (base, 1, 0.85, (0.1, 0.1, 0.0, 0.0)),
            (other, 2, 0.80, (0.0, 0.0, 0.0, 0.0)),                    # one class on overlapping boxes: one kept
            (other + 2.0, 2, 0.75, (0.2, -0.1, 0.1, 0.0)),
            (np.array([90.0, 70.0, 110.0, 95.0], np.float32), 1, 0.95, (0.3, 0.2, 25.0, 30.0)),   # the dw clamp: clipped on all four sides
            (np.array([5.0, 4.0, 60.0, 50.0], np.float32), 0, 0.62, (-6.0, -7.0, 1.0, 1.5)),      # clipped at the near edges; 0.62 < 0.7
            (np.array([150.0, 110.0, 198.0, 158.0], np.float32), 0, 0.64, (5.0, 6.0, 1.0, 1.0)),  # clipped at the far edges
            (np.array([10.0, 100.0, 50.0, 150.0], np.float32), 1, 0.40, (0.0, 0.0, 0.0, 0.0)),    # below both thresholds
            (np.array([60.0, 10.0, 90.0, 28.0], np.float32), 2, 0.72, (0.0, 0.5, -1.0, 0.5)),
            (np.array([10.0, 10.0, 30.0, 28.0], np.float32), 1, 0.99, (0.0, 0.0, 0.0, 0.0)),
            (np.array([15.0, 60.0, 35.0, 90.0], np.float32), 0, 0.97, (np.nan, 0.0, 0.0, 0.0)),   # a non-finite box: dropped
            (np.array([160.0, 10.0, 190.0, 40.0], np.float32), 2, 0.93, (0.0, 0.0, 0.0, 0.0)),    # beyond n_prop in image 0
        ]
        rows = [[(k, p, dl) for _, k, p, dl in spec] for _ in range(B)]
        for b in range(B):
            for i, (bx, _, _, _) in enumerate(spec):
                prop[b, i] = bx + (3.0 * b if i not in (0, 1) else 0.0)
        n_prop = np.array([R - 1, R], np.int32)
    scores = np.zeros((B, R, C + 1), np.float32)
    deltas = (rs.standard_normal((B, R, D)) * 0.3).astype(np.float32)
    for b in range(B):
        for i, (k, p, dl) in enumerate(rows[b]):
            scores[b, i] = _logits(C, k, p, rs)
            o = 0 if c.agnostic else 4 * k
            deltas[b, i, o:o + 4] = dl
    for a in (scores, deltas, prop, n_prop):
        a.setflags(write=False)
    return scores, deltas, prop, n_prop


def _iou_xyxy(a, b):
    area = lambda q: (q[2] - q[0]) * (q[3] - q[1])
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    return inter / ((area(a) + area(b)) - inter) if (area(a) + area(b)) - inter != 0 else float("nan")


def oracle_post(scores, deltas, prop, n_prop, conf, iou_thr, max_det, frame=FRAME, agnostic=False, box_w=BOX_W, dtype=torch.float64):
    """-> dict(dets [B,max_det,6] float64, counts [B,2], classes / order: per image the kept classes and the kept proposal
    indices, gap_conf, gap_nms)."""
    x, d, pr = (torch.tensor(np.array(a)).to(dtype) for a in (scores, deltas, prop))
    Bn, R, n1 = x.shape
    C = n1 - 1
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    p = torch.softmax(x, -1)[..., :C]
    top = torch.topk(p, min(2, C), -1).values                         # (every row at once: the large cases have thousands)
    best, best_k = p.max(-1)
    lead = (top[..., 0] - top[..., 1]) if C > 1 else torch.full_like(best, math.inf)
    gap_conf, gap_nms = math.inf, math.inf
    dets, counts, classes, order = np.zeros((Bn, max_det, 6)), np.zeros((Bn, 2), np.int32), [], []
    for b in range(Bn):
        npb = R if n_prop is None else int(n_prop[b])
        cand = []
        ok = ~torch.isnan(best[b, :npb])
        if bool(ok.any()):
            gap_conf = min(gap_conf, float((best[b, :npb][ok] - f32(conf)).abs().min()), float(lead[b, :npb][ok].min()))
        for i in (ok & (best[b, :npb] > f32(conf))).nonzero()[:, 0].tolist():
            sc, k = float(best[b, i]), int(best_k[b, i])
            r = pr[b, i]
            dl = d[b, i, (0 if agnostic else 4 * k):(0 if agnostic else 4 * k) + 4]
            w_, h_ = r[2] - r[0], r[3] - r[1]
            cx, cy = r[0] + 0.5 * w_, r[1] + 0.5 * h_
            dw = torch.clamp(dl[2] / f32(box_w[2]), max=DW_MAX if dtype == torch.float64 else float(np.log(np.float32(1000.0) / np.float32(16.0))))
            dh = torch.clamp(dl[3] / f32(box_w[3]), max=DW_MAX if dtype == torch.float64 else float(np.log(np.float32(1000.0) / np.float32(16.0))))
            pcx, pcy = dl[0] / f32(box_w[0]) * w_ + cx, dl[1] / f32(box_w[1]) * h_ + cy
            pw_, ph_ = dw.exp() * w_, dh.exp() * h_
            bx = torch.stack([(pcx - 0.5 * pw_).clamp(0, frame[0]), (pcy - 0.5 * ph_).clamp(0, frame[1]),
                              (pcx + 0.5 * pw_).clamp(0, frame[0]), (pcy + 0.5 * ph_).clamp(0, frame[1])])
            if not bool(torch.isfinite(bx).all()):
                continue
            cand.append((i, sc, k, [float(v) for v in bx]))
        walk = sorted(cand, key=lambda q: (-q[1], q[0]))
        for a_ in range(len(walk)):
            for b_ in range(a_ + 1, len(walk)):
                if walk[a_][2] == walk[b_][2]:
                    v = _iou_xyxy(walk[a_][3], walk[b_][3])
                    if v == v:
                        gap_nms = min(gap_nms, abs(v - iou_thr))
        kept = []
        for q in walk:
            if len(kept) >= max_det:
                break
            if any(e[2] == q[2] and _iou_xyxy(e[3], q[3]) > iou_thr for e in kept):
                continue
            kept.append(q)
        for j, q in enumerate(kept):
            dets[b, j] = q[3] + [q[1], float(q[2])]
        counts[b] = (len(kept), len(cand))
        classes.append([q[2] for q in kept])
        order.append([q[0] for q in kept])
    return dict(dets=dets, counts=counts, classes=classes, order=order, gap_conf=gap_conf, gap_nms=gap_nms)


def post_margins_ok(o) -> bool:
    return o["gap_conf"] > GAP and o["gap_nms"] > GAP


@lru_cache(maxsize=None)
def post_reference(c: PostCase):
    scores, deltas, prop, n_prop = post_inputs(c)
    return oracle_post(scores, deltas, prop, n_prop, c.conf, IOU_THR, c.max_det, agnostic=c.agnostic)


BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0.0)))


def post_exact_inputs():
    """The output stage's exact decisions, which gap_conf keeps the seeded cases away from -> a list of (name, PostCase,
    inputs, dets [B,max_det,6] and counts [B,2] written out by hand).  One proposal (10, 20, 50, 60) with zero deltas decodes
    to itself in every precision: width 40, centre 30, exp(0) * 40 = 40, 30 -+ 20.
      at-conf     C = 1, logits (0, 0): p = exp(0) / (1 + 1) = 0.5 exactly; conf_thr = 0.5 drops it (>)
      below-conf  the same with conf_thr one float32 step below 0.5: kept, score 0.5
      class-tie   C = 4, logits (-200, 0, 0, 0, 0): exp(-200) is 0 in float32 and 2^-288 in float64, where 4 + 2^-288 rounds
                  to 4; classes 1, 2, 3 have p = 1 / 4 exactly and class 1, the lowest, wins: its deltas are zero, those of
                  classes 2 and 3 are not, so the box tells which class the deltas were taken from
    Row 1 of every image is far below the threshold."""
    box = (10.0, 20.0, 50.0, 60.0)
    prop = np.array([[box, (100.0, 100.0, 140.0, 150.0)]] * 2, np.float32)
    n_prop = np.array([2, 2], np.int32)
    out = []
    s1 = np.array([[(0.0, 0.0), (-3.0, 0.0)]] * 2, np.float32)
    d1 = np.zeros((2, 2, 4), np.float32)
    out.append(("at-conf", PostCase("at-conf", 0.5, 2, C=1), (s1, d1, prop, n_prop), np.zeros((2, 2, 6), np.float32),
                np.zeros((2, 2), np.int32)))
    dets = np.zeros((2, 2, 6), np.float32)
    dets[:, 0] = box + (0.5, 0.0)
    out.append(("below-conf", PostCase("below-conf", BELOW_HALF, 2, C=1), (s1, d1, prop, n_prop), dets, np.array([[1, 1]] * 2, np.int32)))
    s4 = np.array([[(-200.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, 5.0)]] * 2, np.float32)
    d4 = np.zeros((2, 2, 16), np.float32)
    d4[:, 0, 0:4] = (3.0, -2.0, 1.0, 1.0)
    d4[:, 0, 8:12] = (5.0, 5.0, 1.0, 1.0)
    d4[:, 0, 12:16] = (-5.0, 2.0, -1.0, 0.5)
    dets = np.zeros((2, 2, 6), np.float32)
    dets[:, 0] = box + (0.25, 1.0)
    out.append(("class-tie", PostCase("class-tie", 0.125, 2, C=4), (s4, d4, prop, n_prop), dets, np.array([[1, 1]] * 2, np.int32)))
    return out


def post_poison_inputs():
    """`conf-0.5` with a row of NaN logits (row 8) and a +inf logit (row 9) in image 0 -> (case, clean inputs, poisoned inputs)."""
    c = POST_CASES[0]
    scores, deltas, prop, n_prop = post_inputs(c)
    bad = np.array(scores)
    bad[0, 8] = NAN
    bad[0, 9, 1] = float("inf")
    return c, (scores, deltas, prop, n_prop), (bad, deltas, prop, n_prop)


def verdict_ref(dets, counts, gt, target, untarget, targeted, iou_match=0.5):
    """The header's verdict for one image, in float64 on the rows given -> bits."""
    n = int(counts[0])
    has_gt = gt is not None and not any(v != v for v in gt)
    if n <= 0:
        te, ua = False, True
    elif has_gt:
        ious = [_iou_xyxy([float(v) for v in dets[j, :4]], [float(v) for v in gt]) for j in range(n)]
        ious = [v if v == v else 0.0 for v in ious]
        j = int(np.argmax(ious))
        match = ious[j] > iou_match
        te = match and int(dets[j, 5]) == target
        ua = not (match and int(dets[j, 5]) == untarget)
    else:
        ks = [int(dets[j, 5]) for j in range(n)]
        te, ua = target in ks, untarget not in ks
    ok = (te and (untarget < 0 or ua)) if targeted else ua
    return (1 if ok else 0) | (2 if te else 0) | (4 if ua else 0)


# ---- the host build -------------------------------------------------------------------------------------------------------
class CSpec(ctypes.Structure):   # GsrRcnnSpec of include/gsraster.h
    _fields_ = [("B", ctypes.c_int32), ("R", ctypes.c_int32), ("M", ctypes.c_int32), ("S", ctypes.c_int32), ("C", ctypes.c_int32),
                ("max_pos", ctypes.c_int32), ("append_gt", ctypes.c_int32), ("seed", ctypes.c_uint32), ("fg_iou", ctypes.c_float),
                ("Cf", ctypes.c_int32), ("Hf", ctypes.c_int32), ("Wf", ctypes.c_int32), ("PH", ctypes.c_int32), ("PW", ctypes.c_int32),
                ("spatial_scale", ctypes.c_float), ("sampling_ratio", ctypes.c_int32),
                ("bw_x", ctypes.c_float), ("bw_y", ctypes.c_float), ("bw_w", ctypes.c_float), ("bw_h", ctypes.c_float),
                ("beta", ctypes.c_float), ("w_cls", ctypes.c_float), ("w_box", ctypes.c_float),
                ("conf_thr", ctypes.c_float), ("iou_thr", ctypes.c_float), ("max_det", ctypes.c_int32),
                ("img_w", ctypes.c_float), ("img_h", ctypes.c_float), ("flags", ctypes.c_uint32)]


def c_spec(**kw) -> CSpec:
    s = CSpec()
    s.B, s.R, s.M, s.S, s.C = B, 1, 1, 1, 1
    s.append_gt, s.fg_iou, s.PH, s.PW, s.spatial_scale = 1, FG_IOU, 14, 14, SCALE
    s.Cf = s.Hf = s.Wf = 1
    s.bw_x, s.bw_y, s.bw_w, s.bw_h = BOX_W
    s.w_cls, s.w_box, s.conf_thr, s.iou_thr, s.max_det = 1.0, 1.0, 0.5, IOU_THR, 1
    s.img_w, s.img_h = FRAME
    for k, v in kw.items():
        assert hasattr(s, k), k
        setattr(s, k, v)
    return s


def host_lib():
    lib = host_build.host_lib("rcnn")
    vp, sp = ctypes.c_void_p, ctypes.POINTER(CSpec)
    lib.rh_sample.argtypes = [sp] + [vp] * 9
    lib.rh_roi_align.argtypes = [sp, vp, vp, vp, ctypes.c_int32, vp]
    lib.rh_roi_align_bwd.argtypes = [sp, vp, vp, ctypes.c_int32, vp, vp]
    lib.rh_roi_align_bwd_scatter.argtypes = [sp, vp, vp, ctypes.c_int32, vp, vp]
    lib.rh_roi_align_bwd_scatter.restype = ctypes.c_int
    lib.rh_loss_f32.argtypes = [sp] + [vp] * 9
    lib.rh_loss_f64.argtypes = [sp] + [vp] * 9
    lib.rh_post.argtypes = [sp] + [vp] * 6
    for fn in (lib.rh_sample, lib.rh_roi_align, lib.rh_roi_align_bwd, lib.rh_loss_f32, lib.rh_loss_f64, lib.rh_post):
        fn.restype = ctypes.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_sample(lib, c: SampleCase, seed=None, inputs=None):
    prop, gt, cls, n_prop = (None if a is None else np.ascontiguousarray(a) for a in (sample_inputs(c) if inputs is None else inputs))
    s = c_spec(B=c.B, R=c.R, M=c.M, S=c.S, C=NC, max_pos=c.max_pos, append_gt=int(c.append_gt), seed=c.seed if seed is None else seed)
    out = dict(idx=np.empty((c.B, c.S), np.int32), rois=np.empty((c.B, c.S, 4), np.float32), labels=np.empty((c.B, c.S), np.int32),
               gt_row=np.empty((c.B, c.S), np.int32), counts=np.empty((c.B, 2), np.int32))
    assert lib.rh_sample(ctypes.byref(s), _p(prop), _p(n_prop), _p(gt), _p(cls), _p(out["idx"]), _p(out["rois"]), _p(out["labels"]),
                         _p(out["gt_row"]), _p(out["counts"])) == 0
    return out


def host_roi(lib, c: RoiCase, inputs=None):
    feat, gp, rois, n_roi = (np.ascontiguousarray(a) for a in (roi_case_inputs(c) if inputs is None else inputs))
    s = c_spec(B=feat.shape[0], S=rois.shape[1], Cf=c.Cf, Hf=c.Hf, Wf=c.Wf, PH=c.PH, PW=c.PW, spatial_scale=c.scale, sampling_ratio=c.ratio)
    pooled, gf = np.empty(gp.shape, np.float32), np.zeros(feat.shape, np.float32)
    assert lib.rh_roi_align(ctypes.byref(s), _p(feat), _p(rois), _p(n_roi), 2, _p(pooled)) == 0
    assert lib.rh_roi_align_bwd(ctypes.byref(s), _p(rois), _p(n_roi), 2, _p(gp), _p(gf)) == 0
    scatter = np.zeros(feat.shape, np.float32)                          # the same sum, every sample's shares added one by one
    assert lib.rh_roi_align_bwd_scatter(ctypes.byref(s), _p(rois), _p(n_roi), 2, _p(gp), _p(scatter)) == 0
    return dict(pooled=pooled, grad_features=gf, scatter=scatter)


def host_loss(lib, c: LossCase, double=False, want_grad=True, inputs=None):
    i = loss_inputs(c) if inputs is None else inputs
    ft = np.float64 if double else np.float32
    x, d, r, gb = (np.ascontiguousarray(i[k], dtype=ft) for k in ("scores", "deltas", "rois", "gt_boxes"))
    lb, gr = np.ascontiguousarray(i["labels"]), np.ascontiguousarray(i["gt_row"])
    s = c_spec(B=c.B, S=c.S, M=c.M, C=c.C, beta=c.beta, w_cls=c.w[0], w_box=c.w[1], flags=1 if c.agnostic else 0)
    loss = np.empty(3, ft)
    gs, gd = (np.empty_like(x), np.empty_like(d)) if want_grad else (None, None)
    fn = lib.rh_loss_f64 if double else lib.rh_loss_f32
    assert fn(ctypes.byref(s), _p(x), _p(d), _p(r), _p(lb), _p(gr), _p(gb), _p(loss), _p(gs), _p(gd)) == 0
    return dict(loss=loss, grad_scores=gs, grad_deltas=gd)


def host_post(lib, c: PostCase, inputs=None):
    scores, deltas, prop, n_prop = (np.ascontiguousarray(a) for a in (post_inputs(c) if inputs is None else inputs))
    Bn = scores.shape[0]
    s = c_spec(B=Bn, R=scores.shape[1], C=scores.shape[2] - 1, conf_thr=c.conf, max_det=c.max_det, flags=1 if c.agnostic else 0)
    dets, counts = np.empty((Bn, c.max_det, 6), np.float32), np.empty((Bn, 2), np.int32)
    assert lib.rh_post(ctypes.byref(s), _p(scores), _p(deltas), _p(prop), _p(n_prop), _p(dets), _p(counts)) == 0
    return dict(dets=dets, counts=counts)

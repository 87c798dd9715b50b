"""Cases and oracle of the RPN loss stage (gsr_rpnloss_label, gsr_rpnloss), shared by the CPU and the device tests.

The oracle is written from the formulas of include/gsraster.h (the RPN loss stage), not from the kernels: anchors, a dense
[M,R] IoU matrix, first-maximum rows, the rows' maxima and the low-quality promotion in numpy float64 on the float32
inputs; the keyed sample as Python's sorted() over (key, r); the two losses in torch with autograd for both gradients,
float64 the reference and the same code in float32 the yardstick.  Loss and gradients are compared through
detloss_cases' err / bound: 4 x the yardstick's error, floor 2^-22, never above 1e-3.

Margins.  Every decision the float32 code takes must be one the float64 oracle takes with room to spare, so that the oracle
alone decides the expected integers.  A case is drawn again (next seed) until
  * no consulted IoU (an anchor's best) lies within GAP = 1e-4 of iou_lo or iou_hi,
  * every present row's maximum is either tied exactly (integer geometry) or leads the next distinct value by more than GAP,
  * an anchor's best row leads its runner-up by more than GAP unless the two are exactly equal (the lowest row then wins),
  * |delta - t| of every positive is further than GAP from 0 and from beta,
and margins_ok() is asserted by every test before it compares anything.
"""
import ctypes
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

import detloss_cases as DC
import host_build
from diff_gaussian_rasterization import rpnloss_ops as RO

bound, err = DC.bound, DC.err
GAP = 1e-4
M32 = 0xFFFFFFFF
NAN, INF = float("nan"), float("inf")
ISENT = -77                      # what integer outputs hold before a call
FSENT = 7.5e8                    # what float outputs hold before a call
COMPARED = ("loss", "grad_logits", "grad_deltas")


# ---- the key ---------------------------------------------------------------------------------------------------------------
def mix32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def sample_key(seed: int, b: int, r: int) -> int:
    return mix32((mix32((seed ^ ((b * 0x9E3779B9) & M32)) & M32) + r) & M32)


def sample_keys(seed: int, b: int, R: int) -> np.ndarray:
    """sample_key(seed, b, r) for r < R, vectorised."""
    x = (np.uint64(mix32((seed ^ ((b * 0x9E3779B9) & M32)) & M32)) + np.arange(R, dtype=np.uint64)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Level(NamedTuple):
    cells: Tuple[Tuple[float, float, float, float], ...]      # [A][4]
    stride: int
    hf: int
    wf: int
    offset: float = 0.0


class Case(NamedTuple):
    id: str
    levels: Tuple[Level, ...]
    gt: Optional[tuple] = None          # designed rows: [B][M][4]; None: drawn (n_gt rows per image)
    cls: Optional[tuple] = None         # [B][M]; None: all present
    B: int = 1
    n_gt: int = 2
    gt_size: Tuple[float, float] = (20.0, 60.0)
    batch: int = 256
    quota: int = 128
    beta: float = 0.0
    w: Tuple[float, float] = (1.0, 1.0)
    seed: int = 20240607
    poison: str = ""                    # "", "unsampled", "sampled"
    min_pos: int = -1                   # the oracle must find more positives than this in image 0 (a case's purpose)


def square(s: float):
    return (-s / 2.0, -s / 2.0, s / 2.0, s / 2.0)


def cells(sizes, ratios):
    """generate_cell_anchors in doubles (cast to float32 with the inputs)."""
    out = []
    for s in sizes:
        for r in ratios:
            w = (s * s / r) ** 0.5
            h = r * w
            out.append((-w / 2.0, -h / 2.0, w / 2.0, h / 2.0))
    return tuple(out)


SQ32 = (square(32.0),)
A3 = cells((32.0,), (0.5, 1.0, 2.0))
A15 = cells((16.0, 24.0, 32.0, 48.0, 64.0), (0.5, 1.0, 2.0))
G35 = (Level(SQ32, 16, 5, 7),)
# designed rows on the 5 x 7 grid of 32-pixel squares at stride 16 (anchor (x, y) = [16x - 16, 16y - 16, 16x + 16, 16y + 16])
DESIGNED = (
    ((24, 16, 56, 48), (0, 0, 0, 0)),          # ties anchors (2,2) and (3,2) at 768 / 1280 = 0.6: both promoted out of the ignore band
    ((24, 24, 56, 56), (0, 0, 0, 0)),          # ties four anchors at 576 / 1472 = 0.391
    ((36, 36, 44, 44), (0, 0, 0, 0)),          # an 8-pixel box inside four anchors: 64 / 1024 each, promoted from label 0
    ((500, 500, 520, 520), (0, 0, 0, 0)),      # overlaps no anchor: promotes nothing
    ((24, 16, 56, 48), (24, 16, 56, 48)),      # identical rows: the lowest m
)
DESIGNED_CLS = ((0, -1), (3, -1), (0, -1), (0, -1), (5, 7))

CASES = (
    Case("r1", (Level(SQ32, 16, 1, 1),), gt=(((-10, -12, 14, 16),),), n_gt=1),
    Case("g35-designed", G35, gt=DESIGNED, cls=DESIGNED_CLS, B=5),
    Case("a3-105", (Level(A3, 16, 5, 7),), B=2, n_gt=3, cls=((0, -1, 4), (-1, 2, -3))),
    Case("a15-300", (Level(A15, 16, 4, 5),), B=2, n_gt=2),
    Case("r255", (Level(A3, 8, 5, 17),), n_gt=2),
    Case("r256", (Level(SQ32, 8, 16, 16),), n_gt=2, beta=0.1),
    Case("r257", (Level(SQ32, 8, 1, 257),), n_gt=2, gt_size=(24.0, 40.0)),
    Case("two-levels", (Level(A3, 8, 9, 11), Level(cells((64.0,), (0.5, 1.0, 2.0)), 16, 5, 6)), B=2, n_gt=3, beta=0.1),
    Case("five-levels", tuple(Level(cells((float(16 << l),), (0.5, 1.0, 2.0)), 4 << l, max(1, 24 >> l), max(1, 28 >> l), 0.5 if l == 1 else 0.0)
                              for l in range(5)), B=2, n_gt=4, gt_size=(12.0, 120.0)),
    Case("none-present", (Level(A3, 16, 5, 7),), B=2, n_gt=2, cls=((-1, -1), (-2, -1))),
    Case("quota-8-4", (Level(SQ32, 2, 24, 24),), gt=(((8.0, 8.0, 40.0, 40.0),),), n_gt=1, batch=8, quota=4, min_pos=12),   # 13 positives
    Case("quota-256-128", (Level(SQ32, 2, 60, 100),), n_gt=15, gt_size=(30.0, 34.0), min_pos=128),       # R = 6000: 24 blocks, two select digits and more
    Case("neg-quota", (Level(A3, 4, 20, 25),), B=2, n_gt=2, batch=64, quota=32),                           # R = 1500: the negatives' quota bites
    Case("r69120", (Level(A3, 4, 160, 144),), n_gt=2, gt_size=(24.0, 48.0), batch=512, quota=256),          # index digits above 16 bits decide
    Case("as-one", (Level(((-16.0, -16.0, 16.0, 16.0), (-8.0, -24.0, 8.0, 24.0)), 8, 12, 9),), B=2, n_gt=3, batch=64, quota=32),   # see split_rows
    Case("w-cls-0", (Level(A3, 16, 5, 7),), n_gt=2, w=(0.0, 1.0)),
    Case("w-loc-0", (Level(A3, 16, 5, 7),), n_gt=2, w=(2.0, 0.0), beta=0.1),
    Case("nan-unsampled", (Level(A3, 4, 20, 25), Level(A3, 8, 10, 13)), B=2, n_gt=2, batch=64, quota=32, poison="unsampled"),
    Case("nan-sampled", (Level(A3, 16, 5, 7),), B=2, n_gt=2, poison="sampled"),
)
BY_ID = {c.id: c for c in CASES}


def split_rows(c: Case, ref, h0: int):
    """A one-level case with integer cell anchors -> (the same anchors as two levels, its reference): rows 0 .. h0 - 1 stay,
    the rows from h0 on become a level whose offset is h0 cells -- which moves y where it belongs and x too far, so its cell
    anchors are moved back in x by as much.  All in integers: the anchors are the same floats, in the same flat order."""
    (l,) = c.levels
    back = float(h0 * l.stride)
    moved = tuple((x1 - back, y1, x2 - back, y2) for x1, y1, x2, y2 in l.cells)
    two = c._replace(id=c.id + "-split", levels=(l._replace(hf=h0), Level(moved, l.stride, l.hf - h0, l.wf, float(h0))))
    inp = dict(ref["inp"])
    for k in ("logits", "deltas"):
        (x,) = ref["inp"][k]
        inp[k] = [np.ascontiguousarray(x[:, :, :h0]), np.ascontiguousarray(x[:, :, h0:])]
    return two, dict(inp=inp, lab=ref["lab"])


def total(c: Case) -> int:
    return sum(len(l.cells) * l.hf * l.wf for l in c.levels)


def extent(c: Case):
    """(width, height) in pixels of the largest level's map."""
    return max(l.wf * l.stride for l in c.levels), max(l.hf * l.stride for l in c.levels)


# ---- the oracle: labels ------------------------------------------------------------------------------------------------------
def anchors(c: Case, dtype=np.float64) -> np.ndarray:
    """[R,4] in flat order r = off_l + (y * Wf + x) * A + a; cell anchors and shifts rounded to float32 first, as the inputs are."""
    out = []
    for l in c.levels:
        ca = np.asarray(l.cells, np.float32).astype(dtype)                                   # [A,4]
        s0 = dtype(np.float32(l.offset * l.stride))
        sx = (np.arange(l.wf) * l.stride).astype(dtype) + s0
        sy = (np.arange(l.hf) * l.stride).astype(dtype) + s0
        sh = np.stack(np.broadcast_arrays(sx[None, :], sy[:, None], sx[None, :], sy[:, None]), -1)   # [Hf,Wf,4]
        out.append((sh[:, :, None, :] + ca[None, None, :, :]).reshape(-1, 4))
    return np.concatenate(out, 0)


def pair_iou(gt: np.ndarray, anc: np.ndarray) -> np.ndarray:
    """[M,4], [R,4] -> [M,R]"""
    g, a = gt[:, None, :], anc[None, :, :]
    area_g, area_a = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1]), (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    iw = np.clip(np.minimum(g[..., 2], a[..., 2]) - np.maximum(g[..., 0], a[..., 0]), 0, None)
    ih = np.clip(np.minimum(g[..., 3], a[..., 3]) - np.maximum(g[..., 1], a[..., 1]), 0, None)
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(inter > 0, inter / ((area_g + area_a) - inter), 0.0)


def oracle_labels(c: Case, gt: np.ndarray, cls: np.ndarray, lo=0.3, hi=0.7, dtype=np.float64):
    """-> dict(pre, labels, matched [B,R], counts [B,4], ok: the margins hold, promoted [B]: anchors the low-quality rule raised)."""
    anc = anchors(c, dtype)
    R = anc.shape[0]
    Bn = gt.shape[0]
    pre, labels, matched = (np.zeros((Bn, R), np.int32) for _ in range(3))
    counts = np.zeros((Bn, 4), np.int32)
    ok, promoted_n = True, []
    for b in range(Bn):
        rows = np.nonzero(cls[b] >= 0)[0]
        if len(rows) == 0:
            matched[b] = -1
            promoted_n.append(0)
        else:
            iou = pair_iou(gt[b, rows].astype(dtype), anc)                                    # [m,R]
            best = iou.max(0)
            matched[b] = rows[np.argmax(iou, 0)]                                               # numpy: the first maximum
            p = np.where(best < dtype(np.float32(lo)), 0, np.where(best < dtype(np.float32(hi)), -1, 1)).astype(np.int32)
            ok &= bool((np.abs(best - lo) > GAP).all() and (np.abs(best - hi) > GAP).all())
            if len(rows) > 1:
                top2 = np.sort(iou, 0)[-2:]
                ok &= bool(((top2[1] == top2[0]) | (top2[1] - top2[0] > GAP)).all())
            rowmax = iou.max(1)
            prom = np.zeros(R, bool)
            for i in range(len(rows)):
                if rowmax[i] > 0:
                    tied = iou[i] == rowmax[i]
                    ok &= bool(((iou[i] > rowmax[i] - GAP) == tied).all())
                    prom |= tied
            promoted_n.append(int((prom & (p != 1)).sum()))
            pre[b] = np.where(prom, 1, p)
        keys = sample_keys(c.seed, b, R)
        order = {k: sorted((int(keys[r]), int(r)) for r in np.nonzero(pre[b] == k)[0]) for k in (1, 0)}      # sorted() on (key, r)
        n_pos = min(c.quota, len(order[1]))
        n_neg = min(c.batch - n_pos, len(order[0]))
        labels[b] = -1
        labels[b, [r for _, r in order[1][:n_pos]]] = 1
        labels[b, [r for _, r in order[0][:n_neg]]] = 0
        counts[b] = (len(order[1]), len(order[0]), n_pos, n_neg)
    return dict(pre=pre, labels=labels, matched=matched, counts=counts, ok=ok, promoted=promoted_n)


# ---- the oracle: losses ------------------------------------------------------------------------------------------------------
def flat_head(c: Case, logits, deltas):
    """per-level [B,A,Hf,Wf] / [B,4A,Hf,Wf] tensors -> [B,R] and [B,R,4] in flat anchor order (views: gradients flow back)."""
    xs, ds = [], []
    for l, x, d in zip(c.levels, logits, deltas):
        Bn, A = x.shape[0], len(l.cells)
        xs.append(x.permute(0, 2, 3, 1).reshape(Bn, -1))
        ds.append(d.reshape(Bn, A, 4, l.hf, l.wf).permute(0, 3, 4, 1, 2).reshape(Bn, -1, 4))
    return torch.cat(xs, 1), torch.cat(ds, 1)


def oracle_loss(c: Case, inp, labels, matched, dtype=torch.float64):
    """-> dict(loss [3] = total, cls, loc; grad_logits, grad_deltas: the levels' gradients concatenated flat; res_ok: the
    residual margin)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    logits = [torch.tensor(x).to(dtype).requires_grad_(True) for x in inp["logits"]]
    deltas = [torch.tensor(d).to(dtype).requires_grad_(True) for d in inp["deltas"]]
    x, d = flat_head(c, logits, deltas)
    lb, mt = torch.tensor(labels).long(), torch.tensor(matched).long()
    anc = torch.tensor(anchors(c, np.float64)).to(dtype)
    gt = torch.tensor(inp["gt"]).to(dtype)
    Bn = x.shape[0]
    norm = f32(float(c.batch * Bn))
    bi, ri = (lb >= 0).nonzero(as_tuple=True)
    xv, tv = x[bi, ri], lb[bi, ri].to(dtype)
    s_cls = (xv.clamp(min=0) - xv * tv + torch.log1p(torch.exp(-xv.abs()))).sum()
    bi, ri = (lb == 1).nonzero(as_tuple=True)
    s_loc = torch.zeros((), dtype=dtype)
    res_ok = True
    if len(bi):
        src, dst = anc[ri], gt[bi, mt[bi, ri]]
        sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
        scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
        dw, dh = dst[:, 2] - dst[:, 0], dst[:, 3] - dst[:, 1]
        dcx, dcy = dst[:, 0] + 0.5 * dw, dst[:, 1] + 0.5 * dh
        t = torch.stack([(dcx - scx) / sw, (dcy - scy) / sh, (dw / sw).log(), (dh / sh).log()], -1)
        res = d[bi, ri] - t
        fin = torch.isfinite(res.detach())
        ra = res.detach().abs()[fin]
        res_ok = bool((ra > GAP).all() and ((ra - c.beta).abs() > GAP).all())
        if c.beta > 0:
            bt = f32(c.beta)
            sl = torch.where(res.abs() < bt, 0.5 * res * res / bt, res.abs() - 0.5 * bt)
        else:
            sl = res.abs()
        s_loc = sl.sum()
    cls_term, loc_term = f32(c.w[0]) * s_cls / norm, f32(c.w[1]) * s_loc / norm
    total_ = cls_term + loc_term
    total_.backward()
    g = lambda ts: torch.cat([(t.grad if t.grad is not None else torch.zeros_like(t)).reshape(-1) for t in ts]).detach()
    return dict(loss=torch.stack([total_, cls_term, loc_term]).detach(), grad_logits=g(logits), grad_deltas=g(deltas), res_ok=res_ok)


# ---- inputs, drawn until the margins hold --------------------------------------------------------------------------------------
def _draw(c: Case, attempt: int):
    rs = np.random.RandomState((c.seed + 7919 * attempt) % (2 ** 31))
    Bn, R = c.B, total(c)
    if c.gt is not None:
        gt = np.asarray(c.gt, np.float32)
    else:
        W, H = extent(c)
        size = rs.uniform(c.gt_size[0], c.gt_size[1], (Bn, c.n_gt, 2))
        if c.id == "quota-256-128":                                              # one row per cell of a 3 x 5 grid: none overlaps another
            cx = 20.0 + 38.0 * (np.arange(15) % 5) + rs.uniform(0, 4, (Bn, 15))
            cy = 20.0 + 38.0 * (np.arange(15) // 5) + rs.uniform(0, 4, (Bn, 15))
            size = np.repeat(rs.uniform(c.gt_size[0], c.gt_size[1], (Bn, c.n_gt, 1)), 2, -1)
        else:
            cx, cy = rs.uniform(0.15 * W, 0.85 * W, (Bn, c.n_gt)), rs.uniform(0.15 * H, 0.85 * H, (Bn, c.n_gt))
        gt = np.stack([cx - size[..., 0] / 2, cy - size[..., 1] / 2, cx + size[..., 0] / 2, cy + size[..., 1] / 2], -1).astype(np.float32)
    cls = np.asarray(c.cls, np.int32) if c.cls is not None else np.zeros(gt.shape[:2], np.int32)
    assert gt.shape == (Bn, cls.shape[1], 4), (c.id, gt.shape)
    logits = [rs.normal(0, 2.0, (Bn, len(l.cells), l.hf, l.wf)).astype(np.float32) for l in c.levels]
    deltas = [rs.normal(0, 0.5, (Bn, 4 * len(l.cells), l.hf, l.wf)).astype(np.float32) for l in c.levels]
    return dict(gt=gt, cls=cls, logits=logits, deltas=deltas, R=R)


def _poison(c: Case, inp, labels):
    """NaN and +-inf into the head's outputs, through the flat views.  "unsampled": every logit of an anchor with label -1
    and every delta of an anchor that is not positive; "sampled": one sampled negative's logit NaN, one's +inf, one
    positive's delta NaN -- and the masks of the elements whose anchor is clean."""
    lg = [torch.tensor(x) for x in inp["logits"]]
    dl = [torch.tensor(d) for d in inp["deltas"]]
    x, d = flat_head(c, lg, dl)                                                   # (copies: reshape of a permuted view)
    lb = torch.tensor(labels)
    vals = torch.tensor([NAN, INF, -INF])
    if c.poison == "unsampled":
        un = lb < 0
        x[un] = vals[torch.arange(int(un.sum())) % 3]
        np_ = lb != 1
        d[np_] = vals[torch.arange(int(np_.sum())) % 3][:, None].expand(-1, 4)
        clean_x, clean_d = torch.ones_like(lb, dtype=torch.bool), torch.ones_like(lb, dtype=torch.bool)
    else:
        clean_x, clean_d = torch.ones_like(lb, dtype=torch.bool), torch.ones_like(lb, dtype=torch.bool)
        neg, pos = (lb[0] == 0).nonzero()[:, 0], (lb[0] == 1).nonzero()[:, 0]
        assert len(neg) >= 2 and len(pos) >= 1, c.id
        x[0, neg[0]], x[0, neg[1]] = NAN, INF
        d[0, pos[0], 2] = NAN
        clean_x[0, neg[0]] = clean_x[0, neg[1]] = False
        clean_d[0, pos[0]] = False
    # back to the levels' layouts
    out_x, out_d, mx, md, o = [], [], [], [], 0
    for l in c.levels:
        A, n = len(l.cells), len(l.cells) * l.hf * l.wf
        Bn = x.shape[0]
        unflat = lambda v, k: v[:, o:o + n].reshape(Bn, l.hf, l.wf, A, *([k] if k else [])).permute(*((0, 3, 4, 1, 2) if k else (0, 3, 1, 2))).reshape(Bn, -1, l.hf, l.wf)
        out_x.append(unflat(x, 0).contiguous().numpy())
        out_d.append(unflat(d, 4).contiguous().numpy())
        mx.append(unflat(clean_x, 0).reshape(-1))
        md.append(unflat(clean_d[..., None].expand(-1, -1, 4), 4).reshape(-1))
        o += n
    inp["logits"], inp["deltas"] = out_x, out_d
    inp["clean_logits"], inp["clean_deltas"] = torch.cat(mx), torch.cat(md)


@lru_cache(maxsize=None)
def reference(cid: str):
    """-> dict(inp, lab: oracle_labels, o64, yard, attempt); read-only."""
    c = BY_ID[cid]
    for attempt in range(200):
        inp = _draw(c, attempt)
        lab = oracle_labels(c, inp["gt"], inp["cls"])
        if not lab["ok"] or lab["counts"][0, 0] <= c.min_pos:
            assert c.gt is None or lab["ok"], f"{cid}: a designed case misses its margins"
            continue
        if c.poison:
            _poison(c, inp, lab["labels"])
        o64 = oracle_loss(c, inp, lab["labels"], lab["matched"])
        if not o64["res_ok"]:
            continue
        o32 = oracle_loss(c, inp, lab["labels"], lab["matched"], dtype=torch.float32)
        for a in [inp["gt"], inp["cls"]] + inp["logits"] + inp["deltas"] + [lab[k] for k in ("pre", "labels", "matched", "counts")]:
            a.setflags(write=False)
        masks = dict(loss=None, grad_logits=inp.get("clean_logits"), grad_deltas=inp.get("clean_deltas"))
        yard = {k: masked_err(o32[k], o64[k], masks[k]) for k in COMPARED} if c.poison != "sampled" else \
            {k: masked_err(o32[k], o64[k], masks[k]) for k in COMPARED[1:]}
        return dict(inp=inp, lab=lab, o64=o64, yard=yard, masks=masks, attempt=attempt)
    raise AssertionError(f"{cid}: no draw with margins in 200 attempts")


def masked_err(q, q64, mask=None) -> float:
    q, q64 = torch.as_tensor(q).double().cpu().reshape(-1), torch.as_tensor(q64).double().cpu().reshape(-1)
    if mask is not None:
        q, q64 = q[mask], q64[mask]
    return err(q, q64)


def margins_ok(ref) -> bool:
    return bool(ref["lab"]["ok"] and ref["o64"]["res_ok"])


def check_losses(c: Case, ref, got, who: str):
    """got: dict(loss [3], grad_logits, grad_deltas flat over the levels).  Prints each figure, then -> the list of misses."""
    fails = []
    if c.poison == "sampled":
        g = torch.as_tensor(got["loss"]).double()
        if bool(torch.isfinite(g).any()) or bool(torch.isfinite(ref["o64"]["loss"]).any()):
            fails.append(("loss must be non-finite", g.tolist()))
    for k in COMPARED:
        if k not in ref["yard"]:
            continue
        e, y = masked_err(got[k], ref["o64"][k], ref["masks"][k]), ref["yard"][k]
        print(f"{who} {c.id} {k}: err {e:.3e} yardstick {y:.3e} bound {bound(y):.3e} ratio {e / max(y, 2.0 ** -24):.2f}")
        if not e <= bound(y):
            fails.append((k, e, bound(y)))
    return fails


# ---- the host build ------------------------------------------------------------------------------------------------------------
def host_lib():
    lib = host_build.host_lib("rpnloss")
    lib.rlh_total.restype = ctypes.c_int
    for f in (lib.rlh_label, lib.rlh_loss32, lib.rlh_loss64):
        f.restype = ctypes.c_int
    return lib


def c_spec(c: Case, B=None, M=None):
    geo = [(len(l.cells), l.hf, l.wf, l.stride, float(np.float32(l.offset * l.stride))) for l in c.levels]
    spec = RO.RpnLossSpec(batch_per_image=c.batch, pos_quota=c.quota, seed=c.seed, beta=c.beta, w_cls=c.w[0], w_loc=c.w[1])
    return RO.c_spec(spec, B=c.B if B is None else B, M=M if M is not None else (len(c.gt[0]) if c.gt is not None else c.n_gt), levels=geo)


def cell_arrays(c: Case):
    return [np.ascontiguousarray(np.asarray(l.cells, np.float32)) for l in c.levels]


def _pp(arrays):
    """a host array of pointers to numpy arrays (kept alive by the caller)"""
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_labels(lib, c: Case, ref):
    inp, R = ref["inp"], total(c)
    cs, cl = c_spec(c, M=inp["gt"].shape[1]), cell_arrays(c)
    out = {k: np.full((c.B, R), ISENT, np.int32) for k in ("pre", "labels", "matched")}
    out["counts"] = np.full((c.B, 4), ISENT, np.int32)
    assert lib.rlh_total(ctypes.byref(cs)) == R
    rc = lib.rlh_label(ctypes.byref(cs), _pp(cl), _p(np.ascontiguousarray(inp["gt"])), _p(np.ascontiguousarray(inp["cls"])), _p(out["pre"]),
                       _p(out["labels"]), _p(out["matched"]), _p(out["counts"]))
    assert rc == 0
    return out


def host_loss(lib, c: Case, ref, double=False):
    inp, lab = ref["inp"], ref["lab"]
    cs, cl = c_spec(c, M=inp["gt"].shape[1]), cell_arrays(c)
    lg, dl = [np.ascontiguousarray(x) for x in inp["logits"]], [np.ascontiguousarray(d) for d in inp["deltas"]]
    loss = np.full(3, FSENT, np.float64)
    gl, gd = [np.full(x.shape, FSENT, np.float64) for x in lg], [np.full(d.shape, FSENT, np.float64) for d in dl]
    fn = lib.rlh_loss64 if double else lib.rlh_loss32
    rc = fn(ctypes.byref(cs), _p(np.ascontiguousarray(lab["labels"])), _p(np.ascontiguousarray(lab["matched"])), _pp(lg), _pp(dl), _pp(cl),
            _p(np.ascontiguousarray(inp["gt"])), _p(loss), _pp(gl), _pp(gd))
    assert rc == 0
    return dict(loss=torch.tensor(loss), grad_logits=torch.cat([torch.tensor(g).reshape(-1) for g in gl]),
                grad_deltas=torch.cat([torch.tensor(g).reshape(-1) for g in gd]))

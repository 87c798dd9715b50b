"""Shared by the object-map classifier's tests (not a test module): the cases, the float64 oracle and its float32 twin (the
yardstick), the host build of csrc/gsr_objmap.h, and the comparisons.

Oracle: logits = W.double() @ f.double() + b per pixel; id = the first maximum with a NaN logit never winning, -1 when no
logit compares greater than -inf; conf = softmax(logits)[id]; the cross entropy per image as the mean over the counted
pixels (id >= 0 and target in 0..K-1) with its torch autograd gradient with respect to the map.

Ids are compared where the oracle's decision is safe from float32 rounding.  A float32 logit is a chain of 17 roundings, so
it lies within gamma * a_c of the exact one, gamma = 17 * 2^-24 and a_c = |b_c| + sum_k |W_ck| |f_k|; a pixel is FRAGILE iff
top1 - top2 <= 2 gamma (a_1 + a_2) in the oracle.  margins_ok asserts that at most 1 % of a case's pixels are fragile before
anything is compared.  The exact kind (multiples of 1/8 in [-2, 2]: every partial sum is exact in float32 in any order) has
no fragile pixel by construction, ties included: there the lower class must win at every pixel.

The bound on conf, the terms and the gradient is the project's (detloss_cases.bound / err): four times the float32 oracle's
distance from the float64 one, floor 2^-22, never above 1e-3, on the largest-magnitude-relative error.  Where the oracle is
not finite (a NaN or an infinity in the inputs) the result must be non-finite at exactly those elements.
"""
import ctypes
import functools
from typing import NamedTuple

import numpy as np
import torch

from detloss_cases import bound, err  # noqa: F401  (the project's bound, used as it is)
from host_build import host_lib

CH = 16
GAMMA = 17 * 2.0 ** -24
MAX_FRAGILE = 0.01
SHAPES = [(1, 1, 1, 1), (1, 7, 5, 2), (2, 17, 33, 5), (1, 16, 16, 33), (2, 9, 31, 256), (1, 3, 3, 1024)]
NONFINITE_SHAPES = [(2, 17, 33, 5), (2, 9, 31, 256)]
ALL_IGNORED = {(2, 9, 31, 256): 1}          # shape -> the image whose targets are all ignored
FLOATS = ("conf", "terms", "grad")


class Case(NamedTuple):
    kind: str          # exact | random | nonfinite | nanrow
    shape: tuple       # (B, H, W, K)
    seed: int

    @property
    def id(self):
        return f"{self.kind}-" + "x".join(map(str, self.shape))


def cases():
    out = [Case(kind, s, 11 + 7 * i) for i, s in enumerate(SHAPES) for kind in ("exact", "random")]
    out += [Case(kind, s, 101 + 7 * i) for i, s in enumerate(NONFINITE_SHAPES) for kind in ("nonfinite", "nanrow")]
    return out


@functools.lru_cache(maxsize=None)
def inputs(c: Case):
    """-> dict(objmap [B,16,H,W] f32, weight [K,16] f32, bias [K] f32, target [B,H,W] i32, palette [K,3] u8), numpy."""
    from gsplat_attack.objects import id2rgb
    B, H, W, K = c.shape
    rng = np.random.default_rng(c.seed)
    if c.kind == "exact":
        eighth = lambda *shape: (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)
        f, wt, bs = eighth(B, CH, H, W), eighth(K, CH), eighth(K)
        for k in range(1, K):                                 # deliberate ties: a later class repeats an earlier one
            if rng.random() < 0.3:
                src = int(rng.integers(0, k))
                wt[k], bs[k] = wt[src], bs[src]
    else:
        f = (rng.random((B, CH, H, W)) * rng.random((B, 1, H, W))).astype(np.float32)       # f = u * a
        f[:, :, : max(1, H // 4), : max(1, W // 3)] = 0.0                                    # a block of all-zero pixels
        wt = (rng.standard_normal((K, CH)) * 0.25).astype(np.float32)
        bs = (rng.standard_normal(K) * 0.1).astype(np.float32)
    if c.kind == "nonfinite":                                  # image 0 only: image 1 must not notice
        f[0, 3, H // 2, W // 2] = np.nan                       # a NaN channel
        f[0, 2, H - 1, W - 1] = np.inf                         # two infinities under weights of opposite sign: inf - inf
        f[0, 5, H - 1, W - 1] = np.inf
        wt[0, 2], wt[0, 5] = 0.5, -0.5
        wt[1, 2], wt[1, 5] = 0.5, 0.25                         # ... and one class that goes to +inf there
    if c.kind == "nanrow":
        wt[K // 2] = np.nan                                    # that class never wins
    t = rng.integers(0, K, size=(B, H, W)).astype(np.int32)
    drop = rng.random((B, H, W)) < 0.1
    t[drop] = np.where(rng.random(int(drop.sum())) < 0.5, -1, K).astype(np.int32)
    if c.shape in ALL_IGNORED:
        t[ALL_IGNORED[c.shape]] = -1
    pal = np.stack([id2rgb(i, max(256, K)) for i in range(K)]).astype(np.uint8)
    out = dict(objmap=f, weight=wt, bias=bs, target=t, palette=pal)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def run_arrays(f, wt, bs, t, dtype, upstream=None):
    """The oracle in `dtype` (torch.float64, or torch.float32 for the yardstick) -> dict(ids i32, conf, terms [B,2], grad),
    numpy float64 but for the ids, plus logits (for the margins)."""
    f, wt, bs = (torch.as_tensor(np.array(a)).to(dtype) for a in (f, wt, bs))        # (copies: the inputs are read-only)
    t = torch.as_tensor(np.array(t)).long()
    B, _, H, W = f.shape
    K = wt.shape[0]
    with torch.no_grad():
        logits = torch.einsum("ck,bkhw->bchw", wt, f) + bs.view(1, K, 1, 1)
        clean = torch.where(torch.isnan(logits), torch.full_like(logits, -np.inf), logits)
        m, arg = clean.max(dim=1)
        first = (clean == m.unsqueeze(1)).to(torch.uint8).argmax(dim=1)     # the first maximum
        ids = torch.where(m > -np.inf, first, torch.full_like(first, -1))
        conf = torch.where(ids >= 0, 1.0 / torch.exp(logits - m.unsqueeze(1)).sum(dim=1), torch.zeros_like(m))
        counted = (ids >= 0) & (t >= 0) & (t < K)
        valid = counted.flatten(1).sum(dim=1)
    # what is not counted takes no part: zero features there, so that nothing non-finite leaks through a masked term
    x = torch.where(counted.unsqueeze(1), f, torch.zeros_like(f)).requires_grad_(True)
    lg = torch.einsum("ck,bkhw->bchw", wt, x) + bs.view(1, K, 1, 1)
    ce = -torch.log_softmax(lg, dim=1).gather(1, t.clamp(0, K - 1).unsqueeze(1))[:, 0]
    total = torch.where(counted, ce, torch.zeros_like(ce)).flatten(1).sum(dim=1)
    loss = torch.where(valid > 0, total / valid.clamp(min=1).to(dtype), torch.zeros_like(total))
    up = torch.ones(B, dtype=dtype) if upstream is None else torch.as_tensor(np.asarray(upstream)).to(dtype)
    (loss * up).sum().backward()
    grad = torch.where(counted.unsqueeze(1), x.grad, torch.zeros_like(x.grad))
    return dict(ids=ids.to(torch.int32).numpy(), conf=conf.double().numpy(),
                terms=torch.stack([loss.detach().double(), valid.double()], dim=1).numpy(), grad=grad.double().numpy(),
                logits=logits.double().numpy())


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """-> dict(o64, o32, fragile [B,H,W] bool, yard {name: the float32 oracle's err}).  Computed once per case; read only."""
    x = inputs(c)
    o64 = run_arrays(x["objmap"], x["weight"], x["bias"], x["target"], torch.float64)
    o32 = run_arrays(x["objmap"], x["weight"], x["bias"], x["target"], torch.float32)
    lg = o64["logits"]
    finite_px = np.isfinite(np.where(np.isnan(x["weight"]).any(axis=1)[None, :, None, None], 0.0, lg)).all(axis=1)
    if c.kind == "exact":
        fragile = np.zeros(finite_px.shape, dtype=bool)
    else:
        mag = np.abs(x["bias"]).astype(np.float64)[None, :, None, None] + \
            np.einsum("ck,bkhw->bchw", np.abs(x["weight"]).astype(np.float64), np.abs(x["objmap"]).astype(np.float64))
        clean = np.where(np.isfinite(lg), lg, -np.inf)
        order = np.argsort(-clean, axis=1, kind="stable")[:, :2]
        top = np.take_along_axis(clean, order, axis=1)
        a = np.take_along_axis(np.where(np.isfinite(mag), mag, 0.0), order, axis=1)
        if lg.shape[1] == 1:
            fragile = np.zeros(finite_px.shape, dtype=bool)
        else:
            with np.errstate(invalid="ignore"):                   # (-inf) - (-inf) at a pixel without a finite logit: not fragile
                fragile = finite_px & (top[:, 0] - top[:, 1] <= 2 * GAMMA * (a[:, 0] + a[:, 1]))
    yard = {k: masked_err(o32[k], o64[k])[0] for k in FLOATS}
    for d in (o64, o32):
        for v in d.values():
            v.setflags(write=False)
    return dict(o64=o64, o32=o32, fragile=fragile, yard=yard)


def margins_ok(c: Case) -> bool:
    r = reference(c)
    n = int(r["fragile"].sum())
    print(f"{c.id}: {n} fragile pixels of {r['fragile'].size}")
    return n <= MAX_FRAGILE * r["fragile"].size


def masked_err(got, want):
    """(err over the elements where the oracle is finite, the two finite masks agree)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    same = bool((np.isfinite(got) == fin).all())
    if not fin.any():
        return 0.0, same
    return err(np.where(fin, got, 0.0), np.where(fin, want, 0.0)), same


def check(got: dict, c: Case, what: str):
    """got: ids and any of conf / terms / grad (numpy or tensors) -> the list of failures against the oracle; prints the figures."""
    r = reference(c)
    as_np = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    fails = []
    ids = as_np(got["ids"]).reshape(r["o64"]["ids"].shape)
    solid = ~r["fragile"]
    wrong = int((ids[solid] != r["o64"]["ids"][solid]).sum())
    if wrong:
        fails.append((what, "ids", wrong))
    for k in FLOATS:
        if got.get(k) is None:
            continue
        want = r["o64"][k]
        g = as_np(got[k]).reshape(want.shape)
        if k != "terms" and r["fragile"].any():               # a fragile pixel may have picked the runner-up: its own figures
            keep = solid if k == "conf" else np.broadcast_to(solid[:, None], want.shape)
            g, want = np.where(keep, g, 0.0), np.where(keep, want, 0.0)
        e, same = masked_err(g, want)
        b = bound(r["yard"][k])
        print(f"{what} {k}: err {e:.3e} yardstick {r['yard'][k]:.3e} bound {b:.3e} finite masks equal {same}")
        if not same or not e <= b:
            fails.append((what, k, e, b, same))
    return fails


# ---- the host build ---------------------------------------------------------------------------------------------------------
class CSpec(ctypes.Structure):   # GsrObjMapSpec of include/gsraster.h
    _fields_ = [("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("K", ctypes.c_int32), ("flags", ctypes.c_uint32)]


@functools.lru_cache(maxsize=None)
def _host():
    lib = host_lib("objmap")
    lib.oh_objmap.restype = ctypes.c_int
    lib.oh_objmap.argtypes = [ctypes.c_void_p] * 12
    lib.oh_limits.restype = None
    lib.oh_limits.argtypes = [ctypes.c_void_p]
    return lib


def host_limits():
    out = (ctypes.c_int32 * 4)()
    _host().oh_limits(out)
    return list(out)


def host_arrays(f, wt, bs, t=None, pal=None, conf=True, stats=True, paint=True, terms=True, grad=True):
    """oh_objmap on numpy arrays -> dict(ids, conf, stats, paint, terms, grad); what was not asked for is None."""
    f, wt, bs = (np.ascontiguousarray(a, dtype=np.float32) for a in (f, wt, bs))
    B, _, H, W = f.shape
    K = wt.shape[0]
    loss = terms or grad
    t = np.ascontiguousarray(t, dtype=np.int32) if loss else None
    pal = np.ascontiguousarray(pal, dtype=np.uint8) if paint else None
    out = dict(ids=np.full((B, H, W), -7, np.int32),
               conf=np.full((B, H, W), -7, np.float32) if conf else None,
               stats=np.full((B, K, 5), -7, np.int32) if stats else None,
               paint=np.full((B, H, W, 3), 7, np.uint8) if paint else None,
               terms=np.full((B, 2), -7, np.float32) if terms else None,
               grad=np.full((B, CH, H, W), -7, np.float32) if grad else None)
    ptr = lambda a: a.ctypes.data if a is not None else None
    cs = CSpec(B, H, W, K, 1 if loss else 0)
    rc = _host().oh_objmap(ctypes.addressof(cs), ptr(f), ptr(wt), ptr(bs), ptr(t), ptr(pal), ptr(out["ids"]), ptr(out["conf"]),
                           ptr(out["stats"]), ptr(out["paint"]), ptr(out["terms"]), ptr(out["grad"]))
    assert rc == 0, rc
    return out


@functools.lru_cache(maxsize=None)
def host_run(c: Case):
    x = inputs(c)
    out = host_arrays(x["objmap"], x["weight"], x["bias"], x["target"], x["palette"])
    for v in out.values():
        v.setflags(write=False)
    return out


def recount(ids, K):
    """[B,H,W] ids -> [B,K,5] (count, x0, y0, x1, y1), right / lower exclusive, five zeros for an absent class: numpy."""
    B = ids.shape[0]
    out = np.zeros((B, K, 5), dtype=np.int32)
    for b in range(B):
        for k in np.unique(ids[b]):
            if k < 0:
                continue
            ys, xs = np.nonzero(ids[b] == k)
            out[b, k] = (len(ys), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return out


# ---- the two-object scene of the group_bboxes test -----------------------------------------------------------------------------
SCENE_SIZE = 64
SCENE_THRESHOLD = 0.1        # the classifier gives a pixel to object c iff object c's composited share exceeds this (and the other's)
SOLO_ALPHA = 0.09            # benign_bboxes' alpha threshold for the solo render: just below, so that rounding cannot matter


def two_object_scene(device):
    """-> (full model, [object 1 alone, object 2 alone], camera, (weight [3,16], bias [3])).  Two opaque blobs of 150 Gaussians
    side by side, object 2 nearer to the camera and overlapping object 1's right edge.  Object c's Gaussians carry the
    one-hot feature e_c, so the composited map's channel c is that object's share of the pixel -- at most its solo alpha:
    an occluder only removes from it.  Classes: 0 = background (logit 1), c = 1, 2 (logit share_c / SCENE_THRESHOLD)."""
    from gsplat_attack.gaussian_model import GaussianModel
    from gsplat_attack.scenes import hydrant, make_scene
    a = hydrant(300, seed=5)
    first = torch.arange(300) < 150
    xyz = a["xyz"] * 0.5
    xyz[first] += torch.tensor([-0.15, 0.0, 0.0])
    xyz[~first] += torch.tensor([0.22, 0.0, -0.3])
    obj = torch.zeros(300, 1, CH)
    obj[first, 0, 1] = 1.0
    obj[~first, 0, 2] = 1.0
    a.update(xyz=xyz, objects_dc=obj, opacity=torch.full((300, 1), 3.0))
    pick = lambda m: {k: v[m] for k, v in a.items()}
    full = GaussianModel.from_tensors(**a, device=device)
    solos = [GaussianModel.from_tensors(**pick(first), device=device), GaussianModel.from_tensors(**pick(~first), device=device)]
    _, cams, _ = make_scene("hydrant-1k", device=device, width=SCENE_SIZE, height=SCENE_SIZE, n_views=1)
    wt = torch.zeros(3, CH)
    wt[1, 1] = wt[2, 2] = 1.0 / SCENE_THRESHOLD
    return full, solos, cams[0], (wt, torch.tensor([1.0, 0.0, 0.0]))

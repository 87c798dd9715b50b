"""Shared by the image-loss tests (not a test module): the cases, a float64 torch oracle with an autograd gradient, the same
oracle in float32 as the yardstick, and the host build of the kernels' scalar source (tests/host_math/imgloss_host.cpp over
csrc/gsr_imgloss.h).

The oracle is the reference's _ssim restated separably -- the eleven float32 taps widened, rows then columns, zero padding --
with torch's own autograd behind it; l1 and l2 are torch.abs / the square, means per image.  err / bound are detloss_cases'
rule: a quantity may be 4 x as far from the float64 oracle as the float32 oracle is, at least 2^-22, never above 1e-3, all
relative to the quantity's largest magnitude.

Inputs: y uniform in [0,1], x = y + 0.1 * noise with |noise| >= 0.05, except a block of pixels copied from y.  So every
|x - y| is exactly 0 or above GAP: sign(x - y) is the same in float32 and float64 (margins_ok asserts it).  No value the
kernels form from them is subnormal.
"""
import ctypes
from functools import lru_cache
from typing import NamedTuple, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import host_build
from detloss_cases import FLOOR, bound, err  # noqa: F401  (the project's one rule, used by the tests through this module)

GAP = 1e-3
WEIGHTS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.8, 0.0, 0.2), (0.0, 0.0, 0.0))
CLAMP01 = 1
COMPARED = ("terms", "map", "grad")


class CSpec(ctypes.Structure):   # GsrImgLossSpec of include/gsraster.h
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("w_l1", ctypes.c_float), ("w_l2", ctypes.c_float), ("w_ssim", ctypes.c_float), ("flags", ctypes.c_uint32)]


@lru_cache(maxsize=None)
def host_lib():
    lib = host_build.host_lib("imgloss")
    vp = ctypes.c_void_p
    lib.ih_tile.argtypes = [vp, vp, vp]
    lib.ih_tile.restype = None
    lib.ih_imgloss.argtypes = [ctypes.POINTER(CSpec), vp, vp, vp, vp, vp]
    lib.ih_imgloss.restype = ctypes.c_int
    return lib


@lru_cache(maxsize=None)
def header():
    """(TH, TW, the eleven taps as a float32 array), read from csrc/gsr_imgloss.h through the harness."""
    th, tw = ctypes.c_int32(0), ctypes.c_int32(0)
    taps = np.zeros(11, np.float32)
    host_lib().ih_tile(ctypes.byref(th), ctypes.byref(tw), taps.ctypes.data_as(ctypes.c_void_p))
    return int(th.value), int(tw.value), taps


def reference_taps() -> np.ndarray:
    """The reference's gaussian(11, 1.5): exp(-(k - 5)^2 / 4.5) as float32, divided by their float32 sum."""
    from math import exp
    g = torch.tensor([exp(-(k - 5) ** 2 / float(2 * 1.5 ** 2)) for k in range(11)], dtype=torch.float32)
    return (g / g.sum()).numpy()


class Case(NamedTuple):
    name: str
    shape: Tuple[int, int, int, int]
    kind: str = "noise"          # noise | identical | constant | clamp
    clamp: bool = False

    @property
    def id(self):
        return self.name


def shapes():
    th, tw, _ = header()
    return ((1, 1, 1, 1), (1, 1, 7, 5), (1, 3, 11, 12), (2, 3, 37, 45), (2, 3, th + 1, 2 * tw + 1), (1, 4, 2 * th - 1, tw - 1))


GOLDEN_SHAPE = (2, 3, 37, 45)
CONST_X, CONST_Y = 0.5, 0.25
# Two constant images, a pixel more than 5 from every border: mu1 = a S, mu2 = b S, E11 = a^2 S ... with S the window's
# sum, so with S = 1 the variances vanish and map = (2ab + C1) / (a^2 + b^2 + C1) = 0.2501 / 0.3126.  The float32 taps give
# S = 1 - 6.2e-8 (twice the 1-D sum's 3.1e-8), which leaves s1 + s2 = (a^2 + b^2) S (1 - S) = 1.9e-8 beside C2 = 9e-4 and
# 2 s12 = 1.6e-8: the map lies (1 + 1.7e-5) / (1 + 2.2e-5) - 1 = -4.3e-6 from the literal.  CONST_TOL covers that twice.
CONST_MAP = 0.2501 / 0.3126
CONST_TOL = 1e-5


def cases():
    out = [Case("x".join(map(str, s)), s) for s in shapes()]
    out += [Case("identical", (2, 3, 13, 17), "identical"), Case("constant", (1, 2, 23, 40), "constant"),
            Case("clamp", (2, 3, 19, 37), "clamp", True)]
    return tuple(out)


@lru_cache(maxsize=None)
def inputs(c: Case):
    """-> (x, y) float32 numpy [B,C,H,W]."""
    B, C, H, W = c.shape
    g = torch.Generator().manual_seed(1000 + 7 * H + W + 31 * C + B)
    y = torch.rand(c.shape, generator=g, dtype=torch.float32)
    if c.kind == "identical":
        return y.numpy().copy(), y.numpy().copy()
    if c.kind == "constant":
        return np.full(c.shape, CONST_X, np.float32), np.full(c.shape, CONST_Y, np.float32)
    noise = torch.randn(c.shape, generator=g, dtype=torch.float32)
    noise = torch.sign(noise) * (noise.abs() + 0.05)
    if c.kind == "clamp":
        y = 0.2 + 0.6 * y                                   # y well inside [0,1]: the clamp acts on x alone ...
        x = y + 0.6 * noise                                 # ... which leaves [0,1] on both sides
        flat = x.view(-1)
        flat[0], flat[1], flat[2], flat[3] = 0.0, 1.0, -0.0, 1.0     # exactly on the clamp's edges: the mask passes them
        y.view(-1)[4] = 1.5                                 # a reference pixel above 1: clamped, no mask (nothing flows to y)
        y.view(-1)[5] = -0.5
    else:
        x = y + 0.1 * noise
        x[..., : max(1, H // 3), : max(1, W // 2)] = y[..., : max(1, H // 3), : max(1, W // 2)]     # copied pixels: d = 0
        if H * W == 1:
            x = y + 0.1 * noise                             # one pixel: keep a difference
    return x.numpy().copy(), y.numpy().copy()


def margins_ok(c: Case) -> bool:
    x, y = (torch.from_numpy(a).double() for a in inputs(c))
    if c.clamp:
        x, y = x.clamp(0, 1), y.clamp(0, 1)
    d = (x - y).abs()
    d32 = (torch.from_numpy(inputs(c)[0]) - torch.from_numpy(inputs(c)[1])).abs() if not c.clamp else d.float()
    ok = bool(((d == 0) | (d > GAP)).all()) and bool(((d32 == 0) == (d.float() == 0)).all())
    if c.kind == "noise" and c.shape[2] * c.shape[3] > 1:
        ok = ok and bool((d == 0).any()) and bool((d > GAP).any())
    return ok


def window(t: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """win * t per channel: rows (along x) first, then columns, zero padding of 5."""
    C = t.shape[1]
    kx = taps.view(1, 1, 1, 11).expand(C, 1, 1, 11).contiguous()
    ky = taps.view(1, 1, 11, 1).expand(C, 1, 11, 1).contiguous()
    return F.conv2d(F.conv2d(t, kx, padding=(0, 5), groups=C), ky, padding=(5, 0), groups=C)


def ssim_map(x: torch.Tensor, y: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    mu1, mu2 = window(x, taps), window(y, taps)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = window(x * x, taps) - mu1_sq, window(y * y, taps) - mu2_sq, window(x * y, taps) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def run_arrays(x_np, y_np, weights, dtype, clamp=False, upstream=None):
    """The oracle on arrays -> dict(terms [B,4], map, grad) as tensors of `dtype`; upstream: per-image factors on loss_b."""
    taps = torch.from_numpy(header()[2]).to(dtype)
    x = torch.from_numpy(x_np).to(dtype).requires_grad_(True)
    y = torch.from_numpy(y_np).to(dtype)
    xc, yc = (x.clamp(0, 1), y.clamp(0, 1)) if clamp else (x, y)
    m = ssim_map(xc, yc, taps)
    d = xc - yc
    l1, l2, ss = d.abs().mean(dim=(1, 2, 3)), (d * d).mean(dim=(1, 2, 3)), m.mean(dim=(1, 2, 3))
    loss = weights[0] * l1 + weights[1] * l2 + weights[2] * (1 - ss)
    up = torch.ones_like(loss) if upstream is None else torch.as_tensor(upstream, dtype=dtype)
    (loss * up).sum().backward()
    return dict(terms=torch.stack([l1, l2, ss, loss], dim=1).detach(), map=m.detach(), grad=x.grad.detach())


def cancel_scale(x_np, y_np, w_ssim: float) -> float:
    """The largest magnitude among the summands of the SSIM gradient, in float64 from the closed-form derivative maps:
    max over pixels of w_ssim (|win * dmap/dmu1| + |2 x win * dmap/dE11| + |y win * dmap/dE12|) / n.  Where the images are
    identical these cancel to zero (SSIM is at its maximum), so what any float32 evaluation leaves is rounding of summands
    of this size: it is the magnitude the gradient's error is measured against there."""
    taps = torch.from_numpy(header()[2]).double()
    x, y = torch.from_numpy(x_np).double(), torch.from_numpy(y_np).double()
    mu1, mu2 = window(x, taps), window(y, taps)
    e11, e22, e12 = window(x * x, taps), window(y * y, taps), window(x * y, taps)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    a1, a2 = 2 * mu1 * mu2 + C1, 2 * (e12 - mu1 * mu2) + C2
    b1, b2 = mu1 * mu1 + mu2 * mu2 + C1, (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    m = a1 * a2 / (b1 * b2)
    d_e11, d_e12 = -m / b2, 2 * a1 / (b1 * b2)
    d_mu1 = 2 * mu2 * (a2 - a1) / (b1 * b2) + 2 * mu1 * m * (1 / b2 - 1 / b1)
    n = x[0].numel()
    s = window(d_mu1, taps).abs() + (2 * x * window(d_e11, taps)).abs() + (y * window(d_e12, taps)).abs()
    return abs(w_ssim) * s.max().item() / n


def err_to(q, q64, denom=None) -> float:
    """err, or with `denom` the largest absolute difference over that magnitude."""
    if denom is None:
        return err(q, q64)
    return ((torch.as_tensor(q).double().cpu() - torch.as_tensor(q64).double().cpu()).abs().max() / denom).item()


@lru_cache(maxsize=None)
def reference(c: Case, weights):
    """-> dict(o64 = the float64 oracle's outputs, yard = the float32 oracle's err per output, denom = what an output's error
    is divided by where that is not the output's own largest magnitude: the gradient of identical images under an SSIM
    weight, see cancel_scale)."""
    x, y = inputs(c)
    o64, o32 = run_arrays(x, y, weights, torch.float64, c.clamp), run_arrays(x, y, weights, torch.float32, c.clamp)
    denom = {}
    if c.kind == "identical" and weights[2] != 0.0:
        denom["grad"] = cancel_scale(x, y, weights[2])
    return dict(o64=o64, yard={k: err_to(o32[k], o64[k], denom.get(k)) for k in COMPARED}, denom=denom)


def c_spec(shape, weights, clamp=False) -> CSpec:
    B, C, H, W = shape
    return CSpec(B, C, H, W, weights[0], weights[1], weights[2], CLAMP01 if clamp else 0)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_arrays(x, y, weights, clamp=False, want_grad=True, want_map=True):
    """The host build on arrays -> dict(terms, map, grad) as float32 numpy (sentinel-filled first: every element is written)."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    cs = c_spec(x.shape, weights, clamp)
    terms = np.full((x.shape[0], 4), -777.0, np.float32)
    grad = np.full(x.shape, -777.0, np.float32) if want_grad else None
    smap = np.full(x.shape, -777.0, np.float32) if want_map else None
    assert host_lib().ih_imgloss(ctypes.byref(cs), _p(x), _p(y), _p(terms), _p(grad), _p(smap)) == 0
    return dict(terms=terms, map=smap, grad=grad)


@lru_cache(maxsize=None)
def host_run(c: Case, weights):
    x, y = inputs(c)
    return host_arrays(x, y, weights, c.clamp)


def check(got, ref, tag, keys=COMPARED):
    """Every compared output within bound of the float64 oracle; prints each figure first.  -> the list of failures."""
    fails = []
    for k in keys:
        e, yd = err_to(got[k], ref["o64"][k], ref["denom"].get(k)), ref["yard"][k]
        print(f"{tag} {k}: err {e:.3e} yardstick {yd:.3e} bound {bound(yd):.3e}")
        if not e <= bound(yd):
            fails.append((k, e, bound(yd)))
    return fails

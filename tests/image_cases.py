"""Shared by the image front end's tests (not a test module): the cases, the host build of csrc/gsr_image.h
(tests/host_math/image_host.cpp), the float64 torch oracle and the derived error bounds.

Bounds (float32 arithmetic against F.interpolate in float64):

  forward   3 * (ulp32(H) + ulp32(W)) * D + 8 * 2^-24 * max|src|
            D = the largest difference between neighbouring source pixels.  The first term is the float32 rounding of the
            sample coordinate (scale, the product and the subtraction: three roundings at magnitude <= H resp. W, each
            moving the sample by at most one ulp there, hence the value by that times the local slope D); the second is
            the rounding of the three lerps.
  backward  n_max * max|g| * 3 * (ulp32(H) + ulp32(W)) + 64 * 2^-24 * max(A)
            n_max = the largest number of terms a source pixel receives (counted by the host code), each of which carries a
            weight off by the coordinate's rounding; A = the oracle's backward of |g|, the magnitude the roundings of the
            products and of the running sum scale with.

With the per-channel affine (value - mean) * inv_std the forward bound is multiplied by max(inv_std) and grows by
4 * 2^-24 * max|out| (the subtraction, the product, and inv_std's own float32 rounding twice over); in the backward the
incoming gradient is taken as g * inv_std.  The clamp is exact and changes neither bound (D and max|src| are taken of
the clamped source).
"""
import ctypes
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM = os.path.join(ROOT, "tests", "host_math")
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
EPS = 2.0 ** -24


class Case(NamedTuple):
    H: int
    W: int
    rh: int
    rw: int
    out_h: int = 0          # 0: rh (no pad)
    out_w: int = 0
    top: int = 0
    left: int = 0
    pad: float = 0.0
    C: int = 3
    B: int = 1
    clamp: bool = False
    mean: Optional[Tuple[float, ...]] = None
    std: Optional[Tuple[float, ...]] = None
    backward: bool = True

    @property
    def oh(self):
        return self.out_h or self.rh

    @property
    def ow(self):
        return self.out_w or self.rw

    @property
    def inv_std(self):
        # the float32 the library is handed
        return None if self.std is None else tuple(float(np.float32(1.0 / s)) for s in self.std)

    @property
    def id(self):
        s = f"{self.H}x{self.W}-{self.rh}x{self.rw}"
        if self.out_h:
            s += f"-in{self.out_h}x{self.out_w}"
        if self.C != 3 or self.B != 1:
            s += f"-B{self.B}C{self.C}"
        return s + ("-clamp" if self.clamp else "") + ("-norm" if self.mean or self.std else "")


IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))

# (H, W) -> (rh, rw): the plain resizes
RESIZES = [Case(5, 1920, 2, 640), Case(5, 1920, 4, 1422), Case(3, 3840, 3, 641), Case(1080, 7, 1088, 9),
           Case(9, 16, 23, 37), Case(37, 53, 16, 9), Case(12, 20, 24, 40), Case(1, 1, 4, 4), Case(2, 3, 1, 1),
           Case(64, 64, 64, 64), Case(1080, 1920, 360, 640, backward=False)]
# placement with pad, channel counts, clamp, normalisation
COMPOSED = [Case(27, 48, 9, 16, 16, 16, 3, 0, 114 / 255, B=2),
            Case(9, 16, 23, 37, 40, 41, 8, 3, 0.25, C=1),
            Case(37, 53, 16, 9, 17, 12, 1, 2, -1.0, C=4, B=2, clamp=True, mean=(0.1, 0.2, 0.3, 0.4), std=(0.5, 0.25, 2.0, 1.0)),
            Case(12, 20, 24, 40, clamp=True),
            Case(3, 4, 31, 50),          # a strong upscale: the first outputs' coordinates are clamped to 0 and still name pixel 1
            Case(30, 40, 24, 32, **IMAGENET),
            Case(12, 20, 24, 40, 30, 44, 2, 1, 0.5, clamp=True, **IMAGENET)]
# GPU only: a 1080p letterbox and the sources whose width is no multiple of 4 (the 16-byte store's scalar path)
GPU_EXTRA = [Case(1080, 1920, 360, 640, 640, 640, 140, 0, 114 / 255, B=2),
             Case(3, 1921, 2, 641), Case(7, 53, 16, 9, 20, 12, 2, 1, 0.1, clamp=True, **IMAGENET), Case(7, 53, 3, 20)]


def host_lib():
    lib = host_build.host_lib("image")
    i, f, vp, u32 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32
    lib.ih_forward.restype = i
    lib.ih_forward.argtypes = [i] * 10 + [f, vp, vp, u32, vp, vp]
    lib.ih_backward.restype = i
    lib.ih_backward.argtypes = [i] * 10 + [vp, vp, u32, vp, vp, vp, i, ctypes.POINTER(i)]
    lib.ih_to_u8.restype = None
    lib.ih_to_u8.argtypes = [vp, i, i, i, vp]
    lib.ih_axis_sample.restype = None
    lib.ih_axis_sample.argtypes = [i, i, i, vp, vp]
    lib.ih_axis_range.restype = None
    lib.ih_axis_range.argtypes = [i, i, i, vp]
    return lib


def _arr(v):
    return None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float32))


def _p(a):
    return None if a is None else a.ctypes.data


def _dims(c: Case):
    return (c.B, c.C, c.H, c.W, c.oh, c.ow, c.rh, c.rw, c.top, c.left)


def host_forward(lib, c: Case, src: np.ndarray) -> np.ndarray:
    assert src.dtype == np.float32 and src.shape == (c.B, c.C, c.H, c.W) and src.flags.c_contiguous
    dst = np.full((c.B, c.C, c.oh, c.ow), np.nan, np.float32)
    m, s = _arr(c.mean), _arr(c.inv_std)
    assert lib.ih_forward(*_dims(c), c.pad, _p(m), _p(s), 1 if c.clamp else 0, _p(src), _p(dst)) == 0
    return dst


def host_backward(lib, c: Case, src: np.ndarray, g: np.ndarray, into: Optional[np.ndarray] = None):
    """-> (grad_src, n_max).  into: accumulate onto a copy of it."""
    assert g.dtype == np.float32 and g.shape == (c.B, c.C, c.oh, c.ow) and g.flags.c_contiguous
    out = np.full((c.B, c.C, c.H, c.W), np.nan, np.float32) if into is None else into.copy()
    m, s = _arr(c.mean), _arr(c.inv_std)
    n = ctypes.c_int(0)
    assert lib.ih_backward(*_dims(c), _p(m), _p(s), 1 if c.clamp else 0, _p(src), _p(g), _p(out), 0 if into is None else 1,
                           ctypes.byref(n)) == 0
    return out, n.value


def make_inputs(c: Case, seed: int = 0):
    """Uniform-noise image (in [-0.2, 1.2] with exact 0 and 1 sprinkled in under clamp, else [0, 1]) and normal-noise
    gradient, float32 numpy."""
    rng = np.random.default_rng(1000 + seed + 7 * c.H + 13 * c.W + 17 * c.rh + 19 * c.rw)
    src = rng.uniform(0.0, 1.0, (c.B, c.C, c.H, c.W)).astype(np.float32)
    if c.clamp:
        src = (src * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
        flat = src.reshape(-1)
        flat[0::7] = 0.0
        flat[3::11] = 1.0
        if flat.size > 5:
            flat[5] = -0.0
    g = rng.standard_normal((c.B, c.C, c.oh, c.ow)).astype(np.float32)
    return src, g


def torch_compose(x: torch.Tensor, c: Case) -> torch.Tensor:
    """The torch composition the kernels replace, in x's dtype: clamp, F.interpolate, normalise, F.pad."""
    if c.clamp:
        x = x.clamp(0.0, 1.0)
    y = F.interpolate(x, size=(c.rh, c.rw), mode="bilinear", align_corners=False)
    if c.mean is not None or c.std is not None:
        mean = torch.tensor(c.mean or (0.0,) * c.C, dtype=x.dtype).view(1, -1, 1, 1)
        inv = torch.tensor(c.inv_std or (1.0,) * c.C, dtype=x.dtype).view(1, -1, 1, 1)
        y = (y - mean) * inv
    return F.pad(y, (c.left, c.ow - c.left - c.rw, c.top, c.oh - c.top - c.rh), value=c.pad)


def ulp32(v) -> float:
    return float(np.spacing(np.float32(v)))


def _coord(c: Case) -> float:
    return 3.0 * (ulp32(c.H) + ulp32(c.W))


def oracle(c: Case, src: np.ndarray, g: Optional[np.ndarray]):
    """-> (out64, grad64 or None, forward bound, backward bound as a function of n_max)."""
    x = torch.from_numpy(src).double().requires_grad_(g is not None)
    out = torch_compose(x, c)
    s = np.clip(src.astype(np.float64), 0.0, 1.0) if c.clamp else src.astype(np.float64)
    D = max(np.abs(np.diff(s, axis=2)).max(initial=0.0), np.abs(np.diff(s, axis=3)).max(initial=0.0))
    fb = _coord(c) * D + 8 * EPS * np.abs(s).max()
    if c.mean is not None or c.std is not None:
        fb = fb * max(c.inv_std or (1.0,)) + 4 * EPS * float(out.detach().abs().max())
    if g is None:
        return out.detach().numpy(), None, fb, None
    gt = torch.from_numpy(g).double()
    (grad,) = torch.autograd.grad(out, x, gt, retain_graph=True)
    (A,) = torch.autograd.grad(out, x, gt.abs())
    inv = np.asarray(c.inv_std or (1.0,) * c.C, dtype=np.float64).reshape(1, -1, 1, 1)
    gmax = float(np.abs(g.astype(np.float64) * inv).max())
    amax = float(A.abs().max())
    return out.detach().numpy(), grad.numpy(), fb, lambda n_max: n_max * gmax * _coord(c) + 64 * EPS * amax

"""ctypes binding of the fused image losses (include/gsraster.h, GsrImgLossSpec): L1, L2 and SSIM of a batch of images against
reference images and the gradient of their weighted sum with respect to the images, in at most three launches with one
summation order: the same bits on every run.

  imgloss_forward  img, ref [B,C,H,W] -> (terms [B,4] = l1, l2, ssim, loss; grad_img or None; ssim_map or None): the one C call
  image_loss       the same behind torch.autograd -> terms [B,4]; column 3 (loss_b = w_l1 l1_b + w_l2 l2_b + w_ssim (1 - ssim_b))
                   is differentiable with respect to img, the other columns are not; nothing flows to ref (a stated
                   deviation: the reference's ssim differentiates both arguments), and a ref that requires grad raises

Outputs are torch tensors on the inputs' device; the kernels run on the current stream and nothing waits for them.  No
fallback: tensors must live on a HIP device; CPU tensors raise.  The stage has no capability bit: it is present iff the
loaded library exports gsr_imgloss.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional

import torch

from . import _load
from ._ops_common import _f32, _need_device, _ptr, cached_workspace, call

TILE = (16, 32)           # (TH, TW) of csrc/gsr_imgloss.h: one workgroup's tile of a plane
MAX_CHANNELS = 4
CLAMP01 = 1               # GSR_IMGLOSS_CLAMP01
NO_GRAD = 2               # GSR_IMGLOSS_NO_GRAD


class ImgLossSpec(NamedTuple):
    """GsrImgLossSpec without the sizes, which come from the tensors."""
    w_l1: float = 0.0
    w_l2: float = 0.0
    w_ssim: float = 1.0
    clamp: bool = False


class _CImgLossSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("w_l1", ctypes.c_float), ("w_l2", ctypes.c_float), ("w_ssim", ctypes.c_float), ("flags", ctypes.c_uint32)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """The loaded library exports gsr_imgloss: the stage has no capability bit (gsr_query's items are closed)."""
    return hasattr(_load(), "gsr_imgloss")


def c_spec(spec: ImgLossSpec, shape=(1, 1, 1, 1), flags: int = 0) -> _CImgLossSpec:
    B, C, H, W = (int(v) for v in shape)
    for w in (spec.w_l1, spec.w_l2, spec.w_ssim):
        if not math.isfinite(float(w)):
            raise ValueError(f"ImgLossSpec: the weights must be finite, got {spec}")
    return _CImgLossSpec(B, C, H, W, float(spec.w_l1), float(spec.w_l2), float(spec.w_ssim), int(flags) | (CLAMP01 if spec.clamp else 0))


def _shapes(fn: str, img: torch.Tensor, ref: torch.Tensor):
    _need_device(img, fn, "img")
    _need_device(ref, fn, "ref")
    if img.dim() != 4 or tuple(ref.shape) != tuple(img.shape):
        raise ValueError(f"{fn}: img and ref must be [B,C,H,W] of one shape, got {tuple(img.shape)} and {tuple(ref.shape)}")
    if ref.device != img.device:
        raise ValueError(f"{fn}: img and ref must live on one device")
    if not 1 <= int(img.shape[1]) <= MAX_CHANNELS:
        raise ValueError(f"{fn}: 1..{MAX_CHANNELS} channels, got {int(img.shape[1])}")


def imgloss_forward(img: torch.Tensor, ref: torch.Tensor, spec: ImgLossSpec, want_grad: bool = True, want_map: bool = False,
                    ws: Optional[torch.Tensor] = None):
    """-> (terms [B,4], grad_img [B,C,H,W] or None, ssim_map [B,C,H,W] or None), float32; ws: a workspace of the caller's
    (int64 words, as _ops_common.workspace makes) instead of the cached one."""
    _shapes("imgloss", img, ref)
    dev = img.device
    x, y = _f32(img, dev), _f32(ref, dev)
    cs = c_spec(spec, x.shape, 0 if want_grad else NO_GRAD)
    if ws is None:
        # one cached workspace for calls with a gradient and one for calls without: a loop alternates between those two
        ws = cached_workspace("gsr_imgloss_workspace_bytes", cs, dev, variant=not want_grad)
    terms = torch.empty((x.shape[0], 4), dtype=torch.float32, device=dev)
    grad = torch.empty_like(x) if want_grad else None
    smap = torch.empty_like(x) if want_map else None
    call("gsr_imgloss", dev, ctypes.byref(cs), x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel() * 8, terms.data_ptr(), _ptr(grad), _ptr(smap))
    return terms, grad, smap


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, ref, spec, want_map):
        need = img.requires_grad
        terms, grad, smap = imgloss_forward(img, ref, spec, want_grad=need, want_map=want_map)
        ctx.grad, ctx.in_dtype = grad, img.dtype
        parts, loss = terms[:, :3].contiguous(), terms[:, 3].contiguous()
        ctx.mark_non_differentiable(*([parts, smap] if smap is not None else [parts]))
        return (parts, loss, smap) if smap is not None else (parts, loss)

    @staticmethod
    def backward(ctx, g_parts, g_loss, *g_map):
        if ctx.grad is None or g_loss is None:
            return None, None, None, None
        return (ctx.grad * g_loss.to(torch.float32).view(-1, 1, 1, 1)).to(ctx.in_dtype), None, None, None


def image_loss(img: torch.Tensor, ref: torch.Tensor, w_l1: float, w_l2: float, w_ssim: float, clamp: bool = False, want_map: bool = False):
    """img, ref [B,C,H,W] -> terms [B,4] = l1, l2, ssim, loss (with want_map: (terms, ssim_map [B,C,H,W])).  terms[:, 3] is
    differentiable with respect to img: the backward scales the gradient the forward computed by the upstream per-image
    value.  Columns 0..2 and the map carry no gradient."""
    if isinstance(ref, torch.Tensor) and ref.requires_grad:
        raise ValueError("image_loss: ref must not require grad: the loss is differentiated with respect to img alone")
    _shapes("image_loss", img, ref)
    out = _ImageLoss.apply(img, ref, ImgLossSpec(float(w_l1), float(w_l2), float(w_ssim), bool(clamp)), bool(want_map))
    terms = torch.cat([out[0], out[1].unsqueeze(1)], dim=1)
    return (terms, out[2]) if want_map else terms

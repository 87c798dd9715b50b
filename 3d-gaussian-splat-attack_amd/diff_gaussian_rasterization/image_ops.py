"""ctypes bindings of the image front end (include/gsraster.h, capability bit GSR_CAP_IMAGE of gsr_query(3)):

  resample           bilinear resize of [B,C,H,W] into a padded canvas (letterbox), optional clamp to [0,1] and
                     per-channel normalisation; differentiable, the backward is a gather with a fixed summation order:
                     no float atomics, the same bits on every run
  resample_backward  that backward on caller tensors (optionally accumulating)
  to_uint8_hwc       [B,3,H,W] float -> [B,H,W,3] uint8, (x.clamp(0,1) * 255).byte().permute(0,2,3,1)

No fallback: tensors must live on a HIP device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from . import _load
from ._ops_common import _need_device, call, capability

GSR_RESAMPLE_CLAMP01 = 1
GSR_CAP_IMAGE = 1


class ResampleSpec(NamedTuple):
    """Where the resized image goes: [B,C,H,W] -> resized to (rh, rw), placed at (top, left) of [B,C,out_h,out_w]; the rest
    is pad_value (written as given, not normalised).  mean / inv_std: C floats each or None (0 / 1); value ->
    (value - mean[c]) * inv_std[c].  clamp: the source is clamped to [0,1] first."""
    out_h: int
    out_w: int
    rh: int
    rw: int
    top: int = 0
    left: int = 0
    pad_value: float = 0.0
    mean: Optional[Sequence[float]] = None
    inv_std: Optional[Sequence[float]] = None
    clamp: bool = False


class _CResample(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("out_h", ctypes.c_int32), ("out_w", ctypes.c_int32),
                ("rh", ctypes.c_int32), ("rw", ctypes.c_int32), ("top", ctypes.c_int32), ("left", ctypes.c_int32),
                ("pad_value", ctypes.c_float),
                ("mean", ctypes.POINTER(ctypes.c_float)), ("inv_std", ctypes.POINTER(ctypes.c_float)),
                ("flags", ctypes.c_uint32)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """Bit 0 of gsr_query(3): the loaded library has the image front end."""
    return capability(3, GSR_CAP_IMAGE)


def _channel_floats(v, C: int, fn: str, name: str):
    if v is None:
        return None
    vals = [float(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    if len(vals) != C:
        raise ValueError(f"{fn}: {name} has {len(vals)} entries for {C} channels")
    return (ctypes.c_float * C)(*vals)


def _c_spec(spec: ResampleSpec, shape, fn: str):
    """-> (_CResample, keep-alive): the host arrays must outlive the call only (the library copies them into the launch)."""
    B, C, H, W = (int(s) for s in shape)
    mean = _channel_floats(spec.mean, C, fn, "mean")
    inv_std = _channel_floats(spec.inv_std, C, fn, "inv_std")
    fp = ctypes.POINTER(ctypes.c_float)
    cs = _CResample(B, C, H, W, int(spec.out_h), int(spec.out_w), int(spec.rh), int(spec.rw), int(spec.top), int(spec.left),
                    float(spec.pad_value), ctypes.cast(mean, fp) if mean is not None else fp(),
                    ctypes.cast(inv_std, fp) if inv_std is not None else fp(), GSR_RESAMPLE_CLAMP01 if spec.clamp else 0)
    return cs, (mean, inv_std)


def _forward(src: torch.Tensor, spec: ResampleSpec) -> torch.Tensor:
    dst = torch.empty((src.shape[0], src.shape[1], int(spec.out_h), int(spec.out_w)), dtype=torch.float32, device=src.device)
    cs, keep = _c_spec(spec, src.shape, "resample")
    call("gsr_image_resample", src.device, ctypes.byref(cs), src.data_ptr(), dst.data_ptr())
    del keep
    return dst


def resample_backward(grad_dst: torch.Tensor, spec: ResampleSpec, src_shape, src: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """grad_src [B,C,H,W] of `resample` for grad_dst [B,C,out_h,out_w] (gsr_image_resample_backward on the current
    stream).  src: the forward's source, needed under spec.clamp only.  out: written (or, with accumulate, added to)."""
    _need_device(grad_dst, "resample_backward", "grad_dst")
    dev = grad_dst.device
    shape = tuple(int(s) for s in src_shape)
    if len(shape) != 4 or tuple(grad_dst.shape) != (shape[0], shape[1], int(spec.out_h), int(spec.out_w)):
        raise ValueError(f"resample_backward: grad_dst {tuple(grad_dst.shape)} does not match source {shape} and the spec")
    g = grad_dst.detach().to(torch.float32).contiguous()
    s = None
    if spec.clamp:
        if src is None:
            raise ValueError("resample_backward: spec.clamp needs src (the clamp's mask)")
        _need_device(src, "resample_backward", "src")
        s = src.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(s.shape) != shape:
            raise ValueError(f"resample_backward: src {tuple(s.shape)} is not {shape}")
    if out is None:
        if accumulate:
            raise ValueError("resample_backward: accumulate needs `out`")
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        _need_device(out, "resample_backward", "out")
        if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("resample_backward: out must be a contiguous float32 tensor of the source's shape on grad_dst's device")
    cs, keep = _c_spec(spec, shape, "resample_backward")
    call("gsr_image_resample_backward", dev, ctypes.byref(cs), s.data_ptr() if s is not None else None, g.data_ptr(), out.data_ptr(),
         1 if accumulate else 0)
    del keep
    return out


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, spec):
        ctx.spec = spec
        ctx.src_shape = tuple(src.shape)
        ctx.save_for_backward(src if spec.clamp else None)
        return _forward(src, spec)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dst):
        (src,) = ctx.saved_tensors
        return resample_backward(grad_dst, ctx.spec, ctx.src_shape, src=src), None


def resample(src: torch.Tensor, spec: ResampleSpec) -> torch.Tensor:
    """src [B,C,H,W] float32 on a HIP device, 1 <= C <= 4 -> [B,C,spec.out_h,spec.out_w]; differentiable in src."""
    _need_device(src, "resample", "src")
    if src.dim() != 4:
        raise ValueError(f"resample: src must be [B,C,H,W], got {tuple(src.shape)}")
    if src.dtype != torch.float32:
        raise ValueError(f"resample: src must be float32, got {src.dtype}")
    return _Resample.apply(src.contiguous(), spec)


def to_uint8_hwc(images: torch.Tensor) -> torch.Tensor:
    """images [B,3,H,W] (or [3,H,W]) float32 on a HIP device -> [B,H,W,3] ([H,W,3]) uint8, contiguous:
    (images.clamp(0,1) * 255).byte().permute(0,2,3,1), NaN -> 0.  One launch on the current stream."""
    _need_device(images, "to_uint8_hwc", "images")
    single = images.dim() == 3
    x = images.detach()
    if single:
        x = x[None]
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"to_uint8_hwc: images must be [B,3,H,W] or [3,H,W], got {tuple(images.shape)}")
    x = x.to(torch.float32).contiguous()
    B, _, H, W = (int(s) for s in x.shape)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    call("gsr_image_to_u8", x.device, x.data_ptr(), B, H, W, out.data_ptr())
    return out[0] if single else out

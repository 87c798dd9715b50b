"""ctypes binding of the object-map classifier (include/gsraster.h, GsrObjMapSpec): the 1x1 convolution over render()'s
16-channel object map fused with its consumers -- the arg-max id map, its confidence, per-class pixel counts and boxes, a
painted image, and the cross entropy against a target id map with its gradient with respect to the map.  No [K,H,W] logit
tensor is made.

  objmap_forward  objmap [B,16,H,W] (or [16,H,W]: B = 1), weight [K,16] (or the Conv2d's [K,16,1,1]), bias [K] -> ObjMapOut:
                  the one C call
  object_ce       the same behind torch.autograd -> loss [B], the mean cross entropy per image over the pixels it counts;
                  differentiable with respect to the map alone.  The classifier is frozen: a weight, bias or target that
                  requires grad raises.

Outputs are torch tensors on the inputs' device; the kernels run on the current stream and nothing waits for them.  No
fallback: tensors must live on a HIP device; CPU tensors raise.  The stage has no capability bit: it is present iff the
loaded library exports gsr_objmap.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from . import _load
from ._ops_common import _f32, _i32, _need_device, _ptr, cached_workspace, call

CHANNELS = 16             # CH of csrc/gsr_objmap.h
MAX_CLASSES = 1024        # MAX_CLASSES there (= GROUP_MAX_CLASSES)
LOSS = 1                  # GSR_OBJMAP_LOSS


class ObjMapOut(NamedTuple):
    ids: torch.Tensor                 # [B,H,W] int32; -1: no logit compared greater than -inf
    conf: Optional[torch.Tensor]      # [B,H,W] float32
    stats: Optional[torch.Tensor]     # [B,K,5] int32: count, x0, y0, x1, y1 (x1, y1 exclusive; five zeros: no pixel)
    paint: Optional[torch.Tensor]     # [B,H,W,3] uint8
    terms: Optional[torch.Tensor]     # [B,2] float32: mean CE, counted pixels
    grad: Optional[torch.Tensor]      # [B,16,H,W] float32: d terms[b,0] / d objmap


class _CObjMapSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("K", ctypes.c_int32), ("flags", ctypes.c_uint32)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """The loaded library exports gsr_objmap: the stage has no capability bit (gsr_query's items are closed)."""
    return hasattr(_load(), "gsr_objmap")


def c_spec(shape=(1, 1, 1), K: int = 1, flags: int = 0) -> _CObjMapSpec:
    B, H, W = (int(v) for v in shape)
    return _CObjMapSpec(B, H, W, int(K), int(flags))


def _frozen(fn: str, **tensors) -> None:
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise ValueError(f"{fn}: {name} must not require grad: the classifier is frozen and the loss is differentiated "
                             "with respect to the map alone")


def _shapes(fn: str, objmap: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, target, palette):
    for name, t in (("objmap", objmap), ("weight", weight), ("bias", bias)):
        _need_device(t, fn, name)
    if objmap.dim() not in (3, 4) or int(objmap.shape[-3]) != CHANNELS:
        raise ValueError(f"{fn}: objmap must be [B,{CHANNELS},H,W] or [{CHANNELS},H,W], got {tuple(objmap.shape)}")
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight[:, :, 0, 0]
    if weight.dim() != 2 or int(weight.shape[1]) != CHANNELS or tuple(bias.shape) != (int(weight.shape[0]),):
        raise ValueError(f"{fn}: weight must be [K,{CHANNELS}] (or [K,{CHANNELS},1,1]) and bias [K], got {tuple(weight.shape)} and {tuple(bias.shape)}")
    K = int(weight.shape[0])
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"{fn}: 1..{MAX_CLASSES} classes, got {K}")
    x = objmap if objmap.dim() == 4 else objmap.unsqueeze(0)
    B, _, H, W = (int(v) for v in x.shape)
    if target is not None:
        _need_device(target, fn, "target")
        if target.dim() == 2 and objmap.dim() == 3:
            target = target.unsqueeze(0)
        if tuple(target.shape) != (B, H, W) or target.is_floating_point():
            raise ValueError(f"{fn}: target must be integer ids of shape {(B, H, W)}, got {target.dtype} {tuple(target.shape)}")
    if palette is not None:
        _need_device(palette, fn, "palette")
        if tuple(palette.shape) != (K, 3) or palette.dtype != torch.uint8:
            raise ValueError(f"{fn}: palette must be uint8 [{K},3], got {palette.dtype} {tuple(palette.shape)}")
    for name, t in (("weight", weight), ("bias", bias), ("target", target), ("palette", palette)):
        if t is not None and t.device != objmap.device:
            raise ValueError(f"{fn}: objmap and {name} must live on one device")
    return x, weight, target, K


def objmap_forward(objmap: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, *, target: Optional[torch.Tensor] = None,
                   palette: Optional[torch.Tensor] = None, want_conf: bool = False, want_stats: bool = False,
                   want_paint: bool = False, want_terms: Optional[bool] = None, want_grad: bool = False) -> ObjMapOut:
    """-> ObjMapOut(ids, conf, stats, paint, terms, grad); what was not asked for is None.  want_terms defaults to "a target is
    given"; want_paint needs a palette, want_terms and want_grad need a target.  A [16,H,W] map is a batch of one (the
    outputs keep the leading 1)."""
    fn = "objmap_forward"
    _frozen(fn, weight=weight, bias=bias, target=target)
    x, weight, target, K = _shapes(fn, objmap, weight, bias, target, palette)
    want_terms = (target is not None) if want_terms is None else bool(want_terms)
    if (want_terms or want_grad) and target is None:
        raise ValueError(f"{fn}: the loss terms and the gradient need a target")
    if want_paint and palette is None:
        raise ValueError(f"{fn}: want_paint needs a palette")
    dev = x.device
    x, w, b = _f32(x, dev), _f32(weight, dev), _f32(bias, dev)
    loss = want_terms or want_grad
    tgt = _i32(target, dev) if loss else None
    pal = palette.contiguous() if want_paint else None
    B, _, H, W = (int(v) for v in x.shape)
    cs = c_spec((B, H, W), K, LOSS if loss else 0)
    ws = cached_workspace("gsr_objmap_workspace_bytes", cs, dev, variant=loss)   # with a loss / without (which needs none)
    ids = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    conf = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_conf else None
    stats = torch.empty((B, K, 5), dtype=torch.int32, device=dev) if want_stats else None
    paint = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if want_paint else None
    terms = torch.empty((B, 2), dtype=torch.float32, device=dev) if want_terms else None
    grad = torch.empty_like(x) if want_grad else None
    call("gsr_objmap", dev, ctypes.byref(cs), x.data_ptr(), w.data_ptr(), b.data_ptr(), _ptr(tgt), _ptr(pal),
         ws.data_ptr() if ws.numel() else None, ws.numel() * 8, ids.data_ptr(), _ptr(conf), _ptr(stats), _ptr(paint), _ptr(terms), _ptr(grad))
    return ObjMapOut(ids, conf, stats, paint, terms, grad)


class _ObjectCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, objmap, weight, bias, target):
        need = objmap.requires_grad
        out = objmap_forward(objmap, weight, bias, target=target, want_terms=True, want_grad=need)
        ctx.grad, ctx.in_dtype, ctx.in_dim = out.grad, objmap.dtype, objmap.dim()
        return out.terms[:, 0].contiguous()

    @staticmethod
    def backward(ctx, g_loss):
        if ctx.grad is None or g_loss is None:
            return None, None, None, None
        g = ctx.grad * g_loss.to(torch.float32).view(-1, 1, 1, 1)
        return (g if ctx.in_dim == 4 else g[0]).to(ctx.in_dtype), None, None, None


def object_ce(objmap: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """objmap [B,16,H,W] or [16,H,W], target [B,H,W] (or [H,W]) ids -> loss [B]: per image the mean over its counted pixels
    (target in 0..K-1 and an id >= 0) of -log softmax(logits)[target]; 0 for an image without one.  Differentiable with
    respect to objmap: the backward scales the gradient the forward computed by the upstream per-image value."""
    fn = "object_ce"
    _frozen(fn, weight=weight, bias=bias, target=target)
    _shapes(fn, objmap, weight, bias, target, None)
    return _ObjectCE.apply(objmap, weight.detach(), bias.detach(), target)

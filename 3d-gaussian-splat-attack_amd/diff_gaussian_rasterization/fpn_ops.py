"""ctypes binding of the FPN RoI pooler (include/gsraster.h, GsrFpnSpec): every RoI pooled from the one level of a
feature pyramid that its size picks (Detectron2's ROIPooler with assign_boxes_to_levels), in one launch chain, with a
gather-form backward in which a tile walks the RoIs of its own level alone.

  pool_forward   features_list (nl maps [B,Cf,Hf_l,Wf_l]), rois [B,S,4], counts -> (pooled [B,S,Cf,PH,PW], roi_level int32
                 [B,S], level_list int32 [B,nl,S], level_count int32 [B,nl]): the one C call
  pool_backward  grad_pooled, rois, level_list, level_count -> one gradient per level: the one C call
  fpn_pool       the same behind torch.autograd -> pooled, differentiable with respect to every level's features (nothing
                 flows to the RoIs)

Outputs are torch tensors on the inputs' device; the kernels run on the current stream and nothing waits for them.  No
fallback: tensors must live on a HIP device; CPU tensors raise.  The stage has no capability bit: it is present iff the
loaded library exports gsr_fpn_pool.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _load
from ._ops_common import _f32, _need_device, _ptr, call
from .rcnn_ops import MAX_POOL, MAX_SAMPLE

MAX_LEVELS = 5


class FpnSpec(NamedTuple):
    """GsrFpnSpec without the sizes, which come from the tensors.  scales: one spatial_scale (1 / stride) per level; thr: one
    threshold on q = sqrt(area) / canonical_size + 1e-8 per level, entry 0 unused (level_thresholds makes them).  The
    defaults are Detectron2's FPN box head on p2..p5."""
    scales: Tuple[float, ...] = (1.0 / 4.0, 1.0 / 8.0, 1.0 / 16.0, 1.0 / 32.0)
    thr: Tuple[float, ...] = (0.0, 0.5, 1.0, 2.0)
    PH: int = 7
    PW: int = 7
    sampling_ratio: int = 0
    canonical_size: float = 224.0


class _CFpnSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("S", ctypes.c_int32), ("Cf", ctypes.c_int32), ("PH", ctypes.c_int32), ("PW", ctypes.c_int32),
                ("sampling_ratio", ctypes.c_int32), ("nl", ctypes.c_int32),
                ("Hf", ctypes.c_int32 * MAX_LEVELS), ("Wf", ctypes.c_int32 * MAX_LEVELS),
                ("scale", ctypes.c_float * MAX_LEVELS), ("thr", ctypes.c_float * MAX_LEVELS),
                ("canonical_size", ctypes.c_float)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """The loaded library exports gsr_fpn_pool: the stage has no capability bit (gsr_query's items are closed)."""
    return hasattr(_load(), "gsr_fpn_pool")


def level_thresholds(strides: Sequence[int], canonical_level: int = 4) -> Tuple[float, ...]:
    """thr[l] = 2^(log2(strides[0]) + l - canonical_level); entry 0 is unused (0)."""
    k0 = int(round(math.log2(int(strides[0]))))
    return (0.0,) + tuple(2.0 ** (k0 + l - int(canonical_level)) for l in range(1, len(strides)))


def c_spec(spec: FpnSpec, B: int = 1, S: int = 1, Cf: int = 1, sizes: Sequence[Tuple[int, int]] = ((1, 1),)) -> _CFpnSpec:
    nl = len(sizes)
    if not 1 <= nl <= MAX_LEVELS:
        raise ValueError(f"FpnSpec: 1..{MAX_LEVELS} levels, got {nl}")
    if len(spec.scales) != nl or len(spec.thr) != nl:
        raise ValueError(f"FpnSpec: {len(spec.scales)} scales and {len(spec.thr)} thresholds for {nl} levels")
    cs = _CFpnSpec(int(B), int(S), int(Cf), int(spec.PH), int(spec.PW), int(spec.sampling_ratio), nl)
    for l, (h, w) in enumerate(sizes):
        cs.Hf[l], cs.Wf[l], cs.scale[l], cs.thr[l] = int(h), int(w), float(spec.scales[l]), float(spec.thr[l])
    cs.canonical_size = float(spec.canonical_size)
    return cs


def _sizes(fn: str, feat_shapes, rois: torch.Tensor, counts: Optional[torch.Tensor]):
    shapes = [tuple(int(v) for v in s) for s in feat_shapes]
    if not 1 <= len(shapes) <= MAX_LEVELS or any(len(s) != 4 for s in shapes):
        raise ValueError(f"{fn}: 1..{MAX_LEVELS} feature maps [B,Cf,Hf,Wf], got {shapes}")
    B, Cf = shapes[0][0], shapes[0][1]
    if any(s[0] != B or s[1] != Cf for s in shapes):
        raise ValueError(f"{fn}: every level must be [B={B},Cf={Cf},Hf,Wf], got {shapes}")
    if rois.dim() != 3 or rois.shape[0] != B or rois.shape[2] != 4:
        raise ValueError(f"{fn}: rois must be [B,S,4] with B={B}, got {tuple(rois.shape)}")
    stride = 0
    if counts is not None:
        _need_device(counts, fn, "counts")
        if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.shape[0] != B or counts.dim() not in (1, 2):
            raise ValueError(f"{fn}: counts must be a contiguous int32 [B] or [B,k] (column 0 is read)")
        stride = 1 if counts.dim() == 1 else int(counts.shape[1])
    return shapes, B, Cf, int(rois.shape[1]), stride


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def pool_forward(features_list: Sequence[torch.Tensor], rois: torch.Tensor, counts: Optional[torch.Tensor], spec: FpnSpec):
    """-> (pooled [B,S,Cf,PH,PW], roi_level int32 [B,S], level_list int32 [B,nl,S], level_count int32 [B,nl]); the entries of
    level_list beyond a level's count are not written."""
    feats = list(features_list)
    for f in feats:
        _need_device(f, "fpn_pool", "features")
    _need_device(rois, "fpn_pool", "rois")
    shapes, B, Cf, S, stride = _sizes("fpn_pool", [f.shape for f in feats], rois, counts)
    dev = feats[0].device
    fs, r = [_f32(f, dev) for f in feats], _f32(rois, dev)
    cs = c_spec(spec, B=B, S=S, Cf=Cf, sizes=[s[2:] for s in shapes])
    nl = len(fs)
    pooled = torch.empty((B, S, Cf, int(cs.PH), int(cs.PW)), dtype=torch.float32, device=dev)
    roi_level = torch.empty((B, S), dtype=torch.int32, device=dev)
    level_list = torch.empty((B, nl, S), dtype=torch.int32, device=dev)
    level_count = torch.empty((B, nl), dtype=torch.int32, device=dev)
    call("gsr_fpn_pool", dev, ctypes.byref(cs), _ptr_array(fs), r.data_ptr(), _ptr(counts), stride, pooled.data_ptr(),
         roi_level.data_ptr(), level_list.data_ptr(), level_count.data_ptr())
    return pooled, roi_level, level_list, level_count


def pool_backward(grad_pooled: torch.Tensor, rois: torch.Tensor, level_list: torch.Tensor, level_count: torch.Tensor, feat_shapes,
                  spec: FpnSpec, out: Optional[Sequence[torch.Tensor]] = None, accumulate: bool = False) -> List[torch.Tensor]:
    """-> one grad_features [B,Cf,Hf_l,Wf_l] per level; `out` (one tensor per level) with accumulate: added to what they hold."""
    for t, name in ((grad_pooled, "grad_pooled"), (rois, "rois"), (level_list, "level_list"), (level_count, "level_count")):
        _need_device(t, "fpn_pool_backward", name)
    shapes, B, Cf, S, _ = _sizes("fpn_pool_backward", feat_shapes, rois, None)
    dev = grad_pooled.device
    cs = c_spec(spec, B=B, S=S, Cf=Cf, sizes=[s[2:] for s in shapes])
    nl = len(shapes)
    if tuple(grad_pooled.shape) != (B, S, Cf, int(cs.PH), int(cs.PW)):
        raise ValueError(f"fpn_pool_backward: grad_pooled must be {(B, S, Cf, int(cs.PH), int(cs.PW))}, got {tuple(grad_pooled.shape)}")
    for t, shape, name in ((level_list, (B, nl, S), "level_list"), (level_count, (B, nl), "level_count")):
        if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"fpn_pool_backward: {name} must be a contiguous int32 {shape}")
    g, r = _f32(grad_pooled, dev), _f32(rois, dev)
    if out is None:
        if accumulate:
            raise ValueError("fpn_pool_backward: accumulate needs `out`")
        out = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
    else:
        out = list(out)
        if len(out) != nl or any(tuple(o.shape) != s or o.dtype != torch.float32 or not o.is_contiguous() or o.device != dev
                                 for o, s in zip(out, shapes)):
            raise ValueError("fpn_pool_backward: `out` must hold one contiguous float32 [B,Cf,Hf,Wf] per level on the gradient's device")
    call("gsr_fpn_pool_backward", dev, ctypes.byref(cs), r.data_ptr(), level_list.data_ptr(), level_count.data_ptr(), g.data_ptr(),
         _ptr_array(out), 1 if accumulate else 0)
    return out


class _FpnPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, counts, spec, *features):
        pooled, roi_level, level_list, level_count = pool_forward(features, rois, counts, spec)
        ctx.spec = spec
        ctx.feat_shapes = [tuple(f.shape) for f in features]
        ctx.in_dtypes = [f.dtype for f in features]
        ctx.rois, ctx.level_list, ctx.level_count = rois.detach(), level_list, level_count
        return pooled

    @staticmethod
    def backward(ctx, grad_pooled):
        nl = len(ctx.feat_shapes)
        if not any(ctx.needs_input_grad[3:]):
            return (None,) * (3 + nl)
        gs = pool_backward(grad_pooled, ctx.rois, ctx.level_list, ctx.level_count, ctx.feat_shapes, ctx.spec)
        return (None, None, None) + tuple(g.to(dt) if need else None
                                          for g, dt, need in zip(gs, ctx.in_dtypes, ctx.needs_input_grad[3:]))


def fpn_pool(features_list: Sequence[torch.Tensor], rois: torch.Tensor, counts: Optional[torch.Tensor] = None,
             spec: FpnSpec = FpnSpec()) -> torch.Tensor:
    """features_list: one [B,Cf,Hf_l,Wf_l] per level, finest first; rois [B,S,4] in image pixels; counts: None (every row),
    int32 [B], or a Sample's counts [B,2] -> pooled [B,S,Cf,PH,PW], differentiable with respect to every level's features."""
    return _FpnPool.apply(rois, counts, spec, *features_list)

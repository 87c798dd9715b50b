"""ctypes binding of the detector loss stage (include/gsraster.h, capability bit GSR_CAP_DETLOSS of gsr_query(3)): the
anchor-free YOLO detection loss -- task-aligned assigner, BCE, CIoU, DFL -- and its gradient with respect to the head's
raw training output, in four launches with a fixed summation order.

  run          pred [B,64+C,A], levels, gt_boxes [B,M,4], gt_cls [B,M] -> (loss[4] = box, cls, dfl, total; grad_pred or None;
               tgt int32 [B,A]; ts [B,A]): the one C call, nothing differentiable
  detloss      the same behind torch.autograd -> (total, items[3]); the forward makes the one C call, with grad_pred when
               pred requires grad, and the backward returns grad_out * grad_pred

Outputs and the workspace are torch tensors on pred's device; the kernels run on the current stream and nothing waits for
them.  No fallback: tensors must live on a HIP device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _load
from . import _ops_common
from ._ops_common import _f32, _i32, _need_device, _ptr, call, capability

GSR_CAP_DETLOSS = 4
MAX_ROWS = 32
MAX_LEVELS = 5
MAX_TOPK = 16


class DetLossSpec(NamedTuple):
    """GsrDetLossSpec without the sizes, which come from the tensors and the level table."""
    topk: int = 10
    alpha: float = 0.5
    beta: float = 6.0
    w_box: float = 7.5
    w_cls: float = 0.5
    w_dfl: float = 1.5
    reg_max: int = 16


class _CDetLossSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("C", ctypes.c_int32), ("M", ctypes.c_int32), ("nl", ctypes.c_int32),
                ("level_h", ctypes.c_int32 * 5), ("level_w", ctypes.c_int32 * 5), ("level_stride", ctypes.c_float * 5),
                ("reg_max", ctypes.c_int32), ("topk", ctypes.c_int32), ("alpha", ctypes.c_float), ("beta", ctypes.c_float),
                ("w_box", ctypes.c_float), ("w_cls", ctypes.c_float), ("w_dfl", ctypes.c_float), ("flags", ctypes.c_uint32)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """Bit 2 of gsr_query(3): the loaded library has the detector loss stage."""
    return capability(3, GSR_CAP_DETLOSS)


def c_spec(spec: DetLossSpec, levels: Sequence[Tuple[int, int, float]], B: int, C: int, M: int) -> _CDetLossSpec:
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"detloss: {len(levels)} levels (1..{MAX_LEVELS})")
    cs = _CDetLossSpec()
    cs.B, cs.C, cs.M, cs.nl = int(B), int(C), int(M), len(levels)
    cs.A = sum(int(h) * int(w) for h, w, _ in levels)
    for i, (h, w, s) in enumerate(levels):
        cs.level_h[i], cs.level_w[i], cs.level_stride[i] = int(h), int(w), float(s)
    cs.reg_max, cs.topk, cs.alpha, cs.beta = int(spec.reg_max), int(spec.topk), float(spec.alpha), float(spec.beta)
    cs.w_box, cs.w_cls, cs.w_dfl, cs.flags = float(spec.w_box), float(spec.w_cls), float(spec.w_dfl), 0
    return cs


def workspace_bytes(cs: _CDetLossSpec) -> int:
    return _ops_common.workspace_bytes("gsr_detloss_workspace_bytes", cs)


def run(pred: torch.Tensor, levels: Sequence[Tuple[int, int, float]], gt_boxes: torch.Tensor, gt_cls: torch.Tensor,
        spec: DetLossSpec = DetLossSpec(), want_grad: bool = True, want_assignment: bool = True):
    """-> (loss float32 [4], grad_pred [B,64+C,A] or None, tgt int32 [B,A] or None, ts float32 [B,A] or None)."""
    _need_device(pred, "detloss", "pred")
    _need_device(gt_boxes, "detloss", "gt_boxes")
    _need_device(gt_cls, "detloss", "gt_cls")
    if pred.dim() != 3 or pred.shape[1] <= 64:
        raise ValueError(f"detloss: pred must be [B,64+C,A] with C >= 1, got {tuple(pred.shape)}")
    B, K, A = (int(v) for v in pred.shape)
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4 or tuple(gt_cls.shape) != tuple(gt_boxes.shape[:2]):
        raise ValueError(f"detloss: gt_boxes must be [B,M,4] and gt_cls [B,M] with B={B}, got {tuple(gt_boxes.shape)} and "
                         f"{tuple(gt_cls.shape)}")
    dev = pred.device
    x, gb, gc = _f32(pred), _f32(gt_boxes, dev), _i32(gt_cls, dev)
    cs = c_spec(spec, levels, B, K - 64, int(gb.shape[1]))
    if cs.A != A:
        raise ValueError(f"detloss: the levels hold {cs.A} anchors, pred has {A}")
    ws = _ops_common.workspace(workspace_bytes(cs), dev)
    loss = torch.empty((4,), dtype=torch.float32, device=dev)
    grad = torch.empty_like(x) if want_grad else None
    tgt = torch.empty((B, A), dtype=torch.int32, device=dev) if want_assignment else None
    ts = torch.empty((B, A), dtype=torch.float32, device=dev) if want_assignment else None
    call("gsr_detloss", dev, ctypes.byref(cs), x.data_ptr(), gb.data_ptr(), gc.data_ptr(), ws.data_ptr(), ws.numel() * 8,
         loss.data_ptr(), _ptr(grad), _ptr(tgt), _ptr(ts))
    return loss, grad, tgt, ts


class _DetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, levels, gt_boxes, gt_cls, spec):
        need = pred.requires_grad
        loss, grad, _, _ = run(pred, levels, gt_boxes, gt_cls, spec, want_grad=need, want_assignment=False)
        ctx.has_grad = need
        ctx.in_dtype = pred.dtype
        if need:
            ctx.save_for_backward(grad)
        items = loss[:3].clone()
        ctx.mark_non_differentiable(items)
        return loss[3].clone(), items

    @staticmethod
    def backward(ctx, grad_total, _grad_items):
        if not ctx.has_grad:
            return None, None, None, None, None
        (grad,) = ctx.saved_tensors
        return (grad * grad_total).to(ctx.in_dtype), None, None, None, None


def detloss(pred: torch.Tensor, levels: Sequence[Tuple[int, int, float]], gt_boxes: torch.Tensor, gt_cls: torch.Tensor,
            spec: DetLossSpec = DetLossSpec()) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (total, items[3] = box, cls, dfl unweighted); total is differentiable with respect to pred."""
    _need_device(pred, "detloss", "pred")
    return _DetLoss.apply(pred, tuple(tuple(l) for l in levels), gt_boxes, gt_cls, spec)

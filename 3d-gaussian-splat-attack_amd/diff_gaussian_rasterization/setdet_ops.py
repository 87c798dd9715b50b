"""ctypes binding of the set-prediction (DETR-style) detector stage (include/gsraster.h, capability bit GSR_CAP_SETDET of
gsr_query(3)): the one-to-one match of ground-truth rows to queries, DETR's set criterion -- weighted cross-entropy, L1,
GIoU -- with its gradients, and the output stage (softmax, threshold, boxes in query order).

  run          logits [B,Q,C+1], boxes [B,Q,4], gt_boxes [B,M,4], gt_cls [B,M] -> (loss[4] = ce, l1, giou, total; grad_logits
               and grad_boxes or None; match int32 [B,M]; tgt int32 [B,Q]): the one C call, nothing differentiable
  setdet_loss  the same behind torch.autograd -> (total, items[3]); the forward makes the one C call, with the gradients
               when an input requires grad, and the backward returns grad_out * the stored gradients
  postprocess  logits, boxes -> (dets [B,max_det,6] x1 y1 x2 y2 score class, counts [B,2] kept / above the threshold), the
               layout detect_ops.verdict takes

Outputs and the workspace are torch tensors on the logits' device; the kernels run on the current stream and nothing waits
for them.  No fallback: tensors must live on a HIP device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _load
from . import _ops_common
from ._ops_common import _f32, _i32, _need_device, _ptr, call, capability

GSR_CAP_SETDET = 8
MAX_ROWS = 32
MAX_QUERIES = 1024
MAX_CLASSES = 1024


class SetDetSpec(NamedTuple):
    """GsrSetDetSpec without the sizes, which come from the tensors."""
    img_w: float = 1.0
    img_h: float = 1.0
    c_class: float = 1.0
    c_l1: float = 5.0
    c_giou: float = 2.0
    w_ce: float = 1.0
    w_l1: float = 5.0
    w_giou: float = 2.0
    eos_coef: float = 0.1
    conf_thr: float = 0.7
    max_det: Optional[int] = None        # None: Q


class _CSetDetSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("Q", ctypes.c_int32), ("C", ctypes.c_int32), ("M", ctypes.c_int32),
                ("img_w", ctypes.c_float), ("img_h", ctypes.c_float), ("c_class", ctypes.c_float), ("c_l1", ctypes.c_float),
                ("c_giou", ctypes.c_float), ("w_ce", ctypes.c_float), ("w_l1", ctypes.c_float), ("w_giou", ctypes.c_float),
                ("eos_coef", ctypes.c_float), ("conf_thr", ctypes.c_float), ("max_det", ctypes.c_int32), ("flags", ctypes.c_uint32)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """Bit 3 of gsr_query(3): the loaded library has the set-prediction detector stage."""
    return capability(3, GSR_CAP_SETDET)


def c_spec(spec: SetDetSpec, B: int, Q: int, C: int, M: int) -> _CSetDetSpec:
    return _CSetDetSpec(int(B), int(Q), int(C), int(M), float(spec.img_w), float(spec.img_h), float(spec.c_class),
                        float(spec.c_l1), float(spec.c_giou), float(spec.w_ce), float(spec.w_l1), float(spec.w_giou),
                        float(spec.eos_coef), float(spec.conf_thr), int(Q if spec.max_det is None else spec.max_det), 0)


def workspace_bytes(cs: _CSetDetSpec) -> int:
    return _ops_common.workspace_bytes("gsr_setdet_workspace_bytes", cs)


def _heads(fn: str, logits: torch.Tensor, boxes: torch.Tensor) -> Tuple[int, int, int]:
    _need_device(logits, fn, "logits")
    _need_device(boxes, fn, "boxes")
    if logits.dim() != 3 or logits.shape[2] < 2:
        raise ValueError(f"{fn}: logits must be [B,Q,C+1] with C >= 1, got {tuple(logits.shape)}")
    if tuple(boxes.shape) != (logits.shape[0], logits.shape[1], 4):
        raise ValueError(f"{fn}: boxes must be [B,Q,4] with the logits' B and Q, got {tuple(boxes.shape)}")
    return int(logits.shape[0]), int(logits.shape[1]), int(logits.shape[2]) - 1


def run(logits: torch.Tensor, boxes: torch.Tensor, gt_boxes: torch.Tensor, gt_cls: torch.Tensor, spec: SetDetSpec = SetDetSpec(),
        want_grad: bool = True, want_matching: bool = True):
    """-> (loss float32 [4], grad_logits [B,Q,C+1] or None, grad_boxes [B,Q,4] or None, match int32 [B,M] or None,
    tgt int32 [B,Q] or None)."""
    B, Q, C = _heads("setdet_loss", logits, boxes)
    _need_device(gt_boxes, "setdet_loss", "gt_boxes")
    _need_device(gt_cls, "setdet_loss", "gt_cls")
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4 or tuple(gt_cls.shape) != tuple(gt_boxes.shape[:2]):
        raise ValueError(f"setdet_loss: gt_boxes must be [B,M,4] and gt_cls [B,M] with B={B}, got {tuple(gt_boxes.shape)} and "
                         f"{tuple(gt_cls.shape)}")
    dev = logits.device
    x, bx, gb, gc = _f32(logits), _f32(boxes, dev), _f32(gt_boxes, dev), _i32(gt_cls, dev)
    M = int(gb.shape[1])
    cs = c_spec(spec, B, Q, C, M)
    ws = _ops_common.workspace(workspace_bytes(cs), dev)
    loss = torch.empty((4,), dtype=torch.float32, device=dev)
    gl = torch.empty_like(x) if want_grad else None
    gbx = torch.empty_like(bx) if want_grad else None
    match = torch.empty((B, M), dtype=torch.int32, device=dev) if want_matching else None
    tgt = torch.empty((B, Q), dtype=torch.int32, device=dev) if want_matching else None
    call("gsr_setdet_loss", dev, ctypes.byref(cs), x.data_ptr(), bx.data_ptr(), gb.data_ptr(), gc.data_ptr(), ws.data_ptr(),
         ws.numel() * 8, loss.data_ptr(), _ptr(gl), _ptr(gbx), _ptr(match), _ptr(tgt))
    return loss, gl, gbx, match, tgt


class _SetDetLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, boxes, gt_boxes, gt_cls, spec):
        need = logits.requires_grad or boxes.requires_grad
        loss, gl, gbx, _, _ = run(logits, boxes, gt_boxes, gt_cls, spec, want_grad=need, want_matching=False)
        ctx.has_grad = need
        ctx.in_dtypes = (logits.dtype, boxes.dtype)
        if need:
            ctx.save_for_backward(gl, gbx)
        items = loss[:3].clone()
        ctx.mark_non_differentiable(items)
        return loss[3].clone(), items

    @staticmethod
    def backward(ctx, grad_total, _grad_items):
        if not ctx.has_grad:
            return None, None, None, None, None
        gl, gbx = ctx.saved_tensors
        return ((gl * grad_total).to(ctx.in_dtypes[0]) if ctx.needs_input_grad[0] else None,
                (gbx * grad_total).to(ctx.in_dtypes[1]) if ctx.needs_input_grad[1] else None, None, None, None)


def setdet_loss(logits: torch.Tensor, boxes: torch.Tensor, gt_boxes: torch.Tensor, gt_cls: torch.Tensor,
                spec: SetDetSpec = SetDetSpec()) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (total, items[3] = ce, l1, giou unweighted); total is differentiable with respect to logits and boxes."""
    _heads("setdet_loss", logits, boxes)
    return _SetDetLoss.apply(logits, boxes, gt_boxes, gt_cls, spec)


def postprocess(logits: torch.Tensor, boxes: torch.Tensor, spec: SetDetSpec = SetDetSpec()) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (dets float32 [B,max_det,6]: kept queries in query order, zero rows beyond; counts int32 [B,2]: kept, above the
    threshold)."""
    B, Q, C = _heads("setdet_postprocess", logits, boxes)
    dev = logits.device
    x, bx = _f32(logits), _f32(boxes, dev)
    cs = c_spec(spec, B, Q, C, 1)
    dets = torch.empty((B, int(cs.max_det), 6), dtype=torch.float32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    call("gsr_setdet_postprocess", dev, ctypes.byref(cs), x.data_ptr(), bx.data_ptr(), dets.data_ptr(), counts.data_ptr())
    return dets, counts

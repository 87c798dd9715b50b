"""ctypes binding of the RPN loss stage (include/gsraster.h, GsrRpnLossSpec): the anchors of up to five feature levels
matched against the ground truth (Detectron2's Matcher with low-quality matches), a keyed sample in the place of
subsample_labels' randperm, and the two RPN losses with their gradient in the head's own layouts -- fixed orders
throughout: the same bits on every run.

  label         anchors (one AnchorLevel per level), gt_boxes [B,M,4], gt_cls [B,M] -> Labels(labels, matched, counts,
                prelabels): the one C call gsr_rpnloss_label
  loss_forward  labels, the head's logits / deltas per level -> (loss [3] = total, cls, loc; grad_logits, grad_deltas per
                level or None): the one C call gsr_rpnloss
  rpn_loss      both behind torch.autograd -> (total, terms [2] = cls, loc); total is differentiable with respect to every
                level's logits and deltas, the terms are not

Outputs are torch tensors on the inputs' device; the kernels run on the current stream and nothing waits for them.  No
fallback: tensors must live on a HIP device; CPU tensors raise.  The stage has no capability bit: it is present iff the
loaded library exports gsr_rpnloss.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _load
from ._ops_common import _f32, _i32, _need_device, cached_workspace, call

MAX_LEVELS = 5
MAX_ROWS = 256
MAX_ANCHORS = 1 << 24
MAX_BATCH = 1 << 16


class RpnLossSpec(NamedTuple):
    """GsrRpnLossSpec without the sizes and the levels' geometry, which come from the tensors and the AnchorLevels.  The
    defaults are Detectron2's RPN."""
    batch_per_image: int = 256
    pos_quota: int = 128
    seed: int = 0
    iou_lo: float = 0.3
    iou_hi: float = 0.7
    beta: float = 0.0
    w_cls: float = 1.0
    w_loc: float = 1.0


class AnchorLevel(NamedTuple):
    """One feature level's anchors: cell_anchors [A,4], the stride in pixels, the feature map's (Hf, Wf) and Detectron2's
    anchor offset (0 unless the generator was built with one)."""
    cell_anchors: torch.Tensor
    stride: int
    size: Tuple[int, int]
    offset: float = 0.0


class Labels(NamedTuple):
    """What gsr_rpnloss_label writes: labels int32 [B,R] (1, 0, -1), matched int32 [B,R] (the anchor's best gt row, -1
    without a present row), counts int32 [B,4] = #pos, #neg, n_pos, n_neg; prelabels int32 [B,R] or None."""
    labels: torch.Tensor
    matched: torch.Tensor
    counts: torch.Tensor
    prelabels: Optional[torch.Tensor]


class _CRpnLossSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("M", ctypes.c_int32), ("nl", ctypes.c_int32),
                ("A", ctypes.c_int32 * MAX_LEVELS), ("Hf", ctypes.c_int32 * MAX_LEVELS), ("Wf", ctypes.c_int32 * MAX_LEVELS),
                ("stride", ctypes.c_int32 * MAX_LEVELS), ("shift0", ctypes.c_float * MAX_LEVELS),
                ("batch_per_image", ctypes.c_int32), ("pos_quota", ctypes.c_int32), ("seed", ctypes.c_uint32),
                ("iou_lo", ctypes.c_float), ("iou_hi", ctypes.c_float), ("beta", ctypes.c_float), ("w_cls", ctypes.c_float),
                ("w_loc", ctypes.c_float), ("flags", ctypes.c_uint32)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """The loaded library exports gsr_rpnloss: the stage has no capability bit (gsr_query's items are closed)."""
    return hasattr(_load(), "gsr_rpnloss")


def c_spec(spec: RpnLossSpec, B: int = 1, M: int = 1, levels: Sequence[Tuple[int, int, int, int, float]] = ((1, 1, 1, 1, 0.0),)) -> _CRpnLossSpec:
    """levels: (A, Hf, Wf, stride, shift0) per level."""
    nl = len(levels)
    if not 1 <= nl <= MAX_LEVELS:
        raise ValueError(f"RpnLossSpec: 1..{MAX_LEVELS} levels, got {nl}")
    for v in (spec.iou_lo, spec.iou_hi, spec.beta, spec.w_cls, spec.w_loc):
        if not math.isfinite(float(v)):
            raise ValueError(f"RpnLossSpec: thresholds, beta and weights must be finite, got {spec}")
    cs = _CRpnLossSpec(int(B), int(M), nl)
    for l, (a, h, w, stride, shift0) in enumerate(levels):
        cs.A[l], cs.Hf[l], cs.Wf[l], cs.stride[l], cs.shift0[l] = int(a), int(h), int(w), int(stride), float(shift0)
    cs.batch_per_image, cs.pos_quota, cs.seed = int(spec.batch_per_image), int(spec.pos_quota), int(spec.seed) & 0xFFFFFFFF
    cs.iou_lo, cs.iou_hi, cs.beta, cs.w_cls, cs.w_loc, cs.flags = (float(spec.iou_lo), float(spec.iou_hi), float(spec.beta),
                                                                    float(spec.w_cls), float(spec.w_loc), 0)
    return cs


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _geometry(fn: str, levels: Sequence[AnchorLevel], dev):
    """-> (the cell anchors as float32 on dev, (A, Hf, Wf, stride, shift0) per level)."""
    lvs = [AnchorLevel(*lv) for lv in levels]
    if not 1 <= len(lvs) <= MAX_LEVELS:
        raise ValueError(f"{fn}: 1..{MAX_LEVELS} levels, got {len(lvs)}")
    cells, geo = [], []
    for lv in lvs:
        _need_device(lv.cell_anchors, fn, "cell_anchors")
        if lv.cell_anchors.dim() != 2 or lv.cell_anchors.shape[1] != 4 or lv.cell_anchors.shape[0] < 1:
            raise ValueError(f"{fn}: cell_anchors must be [A,4], got {tuple(lv.cell_anchors.shape)}")
        cells.append(_f32(lv.cell_anchors, dev))
        geo.append((int(lv.cell_anchors.shape[0]), int(lv.size[0]), int(lv.size[1]), int(lv.stride), float(lv.offset) * int(lv.stride)))
    return cells, geo


def _gt(fn: str, gt_boxes: torch.Tensor, gt_cls: Optional[torch.Tensor]):
    _need_device(gt_boxes, fn, "gt_boxes")
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or not 1 <= int(gt_boxes.shape[1]) <= MAX_ROWS:
        raise ValueError(f"{fn}: gt_boxes must be [B,M,4] with M in 1..{MAX_ROWS}, got {tuple(gt_boxes.shape)}")
    if gt_cls is not None:
        _need_device(gt_cls, fn, "gt_cls")
        if tuple(gt_cls.shape) != tuple(gt_boxes.shape[:2]):
            raise ValueError(f"{fn}: gt_cls must be {tuple(gt_boxes.shape[:2])}, got {tuple(gt_cls.shape)}")


def label(levels: Sequence[AnchorLevel], gt_boxes: torch.Tensor, gt_cls: torch.Tensor, spec: RpnLossSpec, want_pre: bool = False,
          ws: Optional[torch.Tensor] = None) -> Labels:
    """The anchors of `levels`, in the head's order, against gt_boxes [B,M,4] / gt_cls [B,M] (negative: the row is absent);
    ws: a workspace of the caller's (int64 words, as _ops_common.workspace makes) instead of the cached one."""
    _gt("rpnloss_label", gt_boxes, gt_cls)
    dev = gt_boxes.device
    cells, geo = _geometry("rpnloss_label", levels, dev)
    B, M = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    gb, gc = _f32(gt_boxes, dev), _i32(gt_cls, dev)
    cs = c_spec(spec, B=B, M=M, levels=geo)
    if ws is None:
        ws = cached_workspace("gsr_rpnloss_workspace_bytes", cs, dev)
    R = sum(a * h * w for a, h, w, _, _ in geo)
    out = Labels(torch.empty((B, R), dtype=torch.int32, device=dev), torch.empty((B, R), dtype=torch.int32, device=dev),
                 torch.empty((B, 4), dtype=torch.int32, device=dev), torch.empty((B, R), dtype=torch.int32, device=dev) if want_pre else None)
    call("gsr_rpnloss_label", dev, ctypes.byref(cs), _ptr_array(cells), gb.data_ptr(), gc.data_ptr(), ws.data_ptr(), ws.numel() * 8,
         out.labels.data_ptr(), out.matched.data_ptr(), out.counts.data_ptr(), out.prelabels.data_ptr() if want_pre else None)
    return out


def _head_outputs(fn: str, logits: Sequence[torch.Tensor], deltas: Sequence[torch.Tensor], levels: Sequence[AnchorLevel]):
    lg, dl = list(logits), list(deltas)
    if len(lg) != len(levels) or len(dl) != len(levels):
        raise ValueError(f"{fn}: {len(lg)} logits and {len(dl)} deltas tensors for {len(levels)} levels")
    for l, (x, d, lv) in enumerate(zip(lg, dl, levels)):
        _need_device(x, fn, "logits")
        _need_device(d, fn, "deltas")
        A, (Hf, Wf) = int(lv.cell_anchors.shape[0]), (int(lv.size[0]), int(lv.size[1]))
        if x.dim() != 4 or tuple(x.shape[1:]) != (A, Hf, Wf) or tuple(d.shape) != (int(x.shape[0]), 4 * A, Hf, Wf) or x.shape[0] != lg[0].shape[0]:
            raise ValueError(f"{fn}: level {l} must be logits [B,{A},{Hf},{Wf}] and deltas [B,{4 * A},{Hf},{Wf}], got {tuple(x.shape)} and {tuple(d.shape)}")
    return lg, dl


def loss_forward(logits: Sequence[torch.Tensor], deltas: Sequence[torch.Tensor], levels: Sequence[AnchorLevel], labels: torch.Tensor,
                 matched: torch.Tensor, gt_boxes: torch.Tensor, spec: RpnLossSpec, want_grad: bool = True, ws: Optional[torch.Tensor] = None):
    """-> (loss [3] = total, cls, loc; grad_logits, grad_deltas: one float32 tensor per level in the input's layout, or None)."""
    levels = [AnchorLevel(*lv) for lv in levels]
    lg, dl = _head_outputs("rpnloss", logits, deltas, levels)
    _gt("rpnloss", gt_boxes, None)
    dev = lg[0].device
    cells, geo = _geometry("rpnloss", levels, dev)
    B, M, R = int(lg[0].shape[0]), int(gt_boxes.shape[1]), sum(a * h * w for a, h, w, _, _ in geo)
    for t, name in ((labels, "labels"), (matched, "matched")):
        _need_device(t, "rpnloss", name)
        if tuple(t.shape) != (B, R) or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"rpnloss: {name} must be a contiguous int32 {(B, R)}")
    if int(gt_boxes.shape[0]) != B:
        raise ValueError(f"rpnloss: gt_boxes must be [B={B},M,4], got {tuple(gt_boxes.shape)}")
    xs, ds, gb = [_f32(x, dev) for x in lg], [_f32(d, dev) for d in dl], _f32(gt_boxes, dev)
    cs = c_spec(spec, B=B, M=M, levels=geo)
    if ws is None:
        ws = cached_workspace("gsr_rpnloss_workspace_bytes", cs, dev)
    loss = torch.empty((3,), dtype=torch.float32, device=dev)
    gl = [torch.empty_like(x) for x in xs] if want_grad else None
    gd = [torch.empty_like(d) for d in ds] if want_grad else None
    call("gsr_rpnloss", dev, ctypes.byref(cs), labels.data_ptr(), matched.data_ptr(), _ptr_array(xs), _ptr_array(ds), _ptr_array(cells),
         gb.data_ptr(), ws.data_ptr(), ws.numel() * 8, loss.data_ptr(), _ptr_array(gl) if want_grad else None,
         _ptr_array(gd) if want_grad else None)
    return loss, gl, gd


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, levels, labels, matched, gt_boxes, spec, nl, *head):
        logits, deltas = head[:nl], head[nl:]
        need = any(t.requires_grad for t in head)
        loss, gl, gd = loss_forward(logits, deltas, levels, labels, matched, gt_boxes, spec, want_grad=need)
        ctx.grads = (gl + gd) if need else None
        ctx.in_dtypes = [t.dtype for t in head]
        total, terms = loss[0].clone(), loss[1:].clone()
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    def backward(ctx, g_total, g_terms):
        none = (None,) * 6
        if ctx.grads is None or g_total is None:
            return none + (None,) * len(ctx.in_dtypes)
        s = g_total.to(torch.float32)
        return none + tuple((g * s).to(dt) if need else None for g, dt, need in zip(ctx.grads, ctx.in_dtypes, ctx.needs_input_grad[6:]))


def rpn_loss(logits: Sequence[torch.Tensor], deltas: Sequence[torch.Tensor], levels: Sequence[AnchorLevel], gt_boxes: torch.Tensor,
             gt_cls: torch.Tensor, spec: RpnLossSpec = RpnLossSpec(), labels: Optional[Labels] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits: one [B,A,Hf,Wf] per level, deltas: one [B,4A,Hf,Wf] per level; -> (total, terms [2] = cls, loc as they enter
    the total).  total is differentiable with respect to every logits and deltas tensor: the backward scales the gradients
    the forward computed by the upstream value.  labels: what `label` returned for the same anchors and ground truth
    (default: computed here)."""
    levels = [AnchorLevel(*lv) for lv in levels]
    lg, dl = _head_outputs("rpn_loss", logits, deltas, levels)
    _gt("rpn_loss", gt_boxes, gt_cls)
    lb = label(levels, gt_boxes, gt_cls, spec) if labels is None else labels
    return _RpnLoss.apply(levels, lb.labels, lb.matched, gt_boxes.detach(), spec, len(levels), *lg, *dl)

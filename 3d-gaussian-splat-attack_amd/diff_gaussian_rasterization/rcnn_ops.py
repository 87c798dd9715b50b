"""ctypes binding of the two-stage (R-CNN-style) detector stage (include/gsraster.h, capability bit GSR_CAP_RCNN of
gsr_query(4)): the deterministic proposal sampler, RoIAlign with a gather-form backward, the box head's loss with its
gradients, and the output stage (softmax, threshold, box decode, the detector output stage's NMS walk).

  sample       proposals [B,R,4], gt_boxes [B,M,4], gt_cls [B,M] -> Sample(idx, rois, labels, gt_row, counts): one C call
  roi_align    features [B,Cf,Hf,Wf], rois [B,S,4], counts -> pooled [B,S,Cf,PH,PW] behind torch.autograd: the backward is
               gsr_roi_align_backward, to the features alone (nothing flows to the RoIs)
  run_loss     scores [B,S,C+1], deltas [B,S,4C] or [B,S,4], a Sample's rois / labels / gt_row, gt_boxes -> (loss[3] = cls,
               box, total; grad_scores and grad_deltas or None): the one C call, nothing differentiable
  rcnn_loss    the same behind torch.autograd -> (total, items[2]); the backward returns grad_out * the stored gradients
  postprocess  scores, deltas, proposals -> (dets [B,max_det,6] x1 y1 x2 y2 score class, counts [B,2] kept / candidates),
               the layout detect_ops.verdict takes

Outputs and the workspace are torch tensors on the inputs' device; the kernels run on the current stream and nothing waits
for them.  No fallback: tensors must live on a HIP device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _load
from . import _ops_common
from ._ops_common import _f32, _i32, _need_device, _ptr, call, capability

GSR_CAP_RCNN = 16
GSR_RCNN_CLASS_AGNOSTIC = 1
MAX_ROWS = 32
MAX_SAMPLE = 1024
MAX_CAND = 4096
MAX_CLASSES = 1024
MAX_POOL = 14


class RcnnSpec(NamedTuple):
    """GsrRcnnSpec without the sizes, which come from the tensors.  The defaults are Detectron2's C4 Faster R-CNN as the
    reference runs it; w_cls = 1, w_box = 0 is what the reference descends on (Detectron2's own sum: 1, 1)."""
    S: int = 512
    max_pos: int = 128
    append_gt: bool = True
    seed: int = 0
    fg_iou: float = 0.5
    PH: int = 14
    PW: int = 14
    spatial_scale: float = 1.0 / 16.0
    sampling_ratio: int = 0
    box_weights: Tuple[float, float, float, float] = (10.0, 10.0, 5.0, 5.0)
    beta: float = 0.0
    w_cls: float = 1.0
    w_box: float = 0.0
    conf_thr: float = 0.5
    iou_thr: float = 0.5
    max_det: int = 100
    img_w: float = 1.0
    img_h: float = 1.0
    class_agnostic: bool = False


class _CRcnnSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("R", ctypes.c_int32), ("M", ctypes.c_int32), ("S", ctypes.c_int32), ("C", ctypes.c_int32),
                ("max_pos", ctypes.c_int32), ("append_gt", ctypes.c_int32), ("seed", ctypes.c_uint32), ("fg_iou", ctypes.c_float),
                ("Cf", ctypes.c_int32), ("Hf", ctypes.c_int32), ("Wf", ctypes.c_int32), ("PH", ctypes.c_int32), ("PW", ctypes.c_int32),
                ("spatial_scale", ctypes.c_float), ("sampling_ratio", ctypes.c_int32),
                ("bw_x", ctypes.c_float), ("bw_y", ctypes.c_float), ("bw_w", ctypes.c_float), ("bw_h", ctypes.c_float),
                ("beta", ctypes.c_float), ("w_cls", ctypes.c_float), ("w_box", ctypes.c_float),
                ("conf_thr", ctypes.c_float), ("iou_thr", ctypes.c_float), ("max_det", ctypes.c_int32),
                ("img_w", ctypes.c_float), ("img_h", ctypes.c_float), ("flags", ctypes.c_uint32)]


class Sample(NamedTuple):
    """What gsr_rcnn_sample writes: idx int32 [B,S] (-1 beyond the count), rois [B,S,4], labels int32 [B,S] (C: background,
    -1 beyond), gt_row int32 [B,S], counts int32 [B,2] = (taken, foreground taken)."""
    idx: torch.Tensor
    rois: torch.Tensor
    labels: torch.Tensor
    gt_row: torch.Tensor
    counts: torch.Tensor


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """Bit 4 of gsr_query(4), the item that holds bits 0..4 (item 3 is closed at bits 0..3, item 4 at these five): the loaded library
    has the two-stage detector stage.  A library without item 4 refuses it: no stage."""
    return capability(4, GSR_CAP_RCNN)


def c_spec(spec: RcnnSpec, B: int = 1, R: int = 1, M: int = 1, C: int = 1, Cf: int = 1, Hf: int = 1, Wf: int = 1,
           S: Optional[int] = None) -> _CRcnnSpec:
    bw = [float(v) for v in spec.box_weights]
    if len(bw) != 4:
        raise ValueError("RcnnSpec: box_weights has four entries (wx, wy, ww, wh)")
    return _CRcnnSpec(int(B), int(R), int(M), int(spec.S if S is None else S), int(C), int(spec.max_pos), 1 if spec.append_gt else 0,
                      int(spec.seed) & 0xffffffff, float(spec.fg_iou), int(Cf), int(Hf), int(Wf), int(spec.PH), int(spec.PW),
                      float(spec.spatial_scale), int(spec.sampling_ratio), bw[0], bw[1], bw[2], bw[3], float(spec.beta),
                      float(spec.w_cls), float(spec.w_box), float(spec.conf_thr), float(spec.iou_thr), int(spec.max_det),
                      float(spec.img_w), float(spec.img_h), GSR_RCNN_CLASS_AGNOSTIC if spec.class_agnostic else 0)


def workspace_bytes(cs: _CRcnnSpec) -> int:
    return _ops_common.workspace_bytes("gsr_rcnn_workspace_bytes", cs)


def sample(proposals: torch.Tensor, gt_boxes: torch.Tensor, gt_cls: torch.Tensor, nc: int, spec: RcnnSpec = RcnnSpec(),
           n_prop: Optional[torch.Tensor] = None) -> Sample:
    """proposals [B,R,4] x1 y1 x2 y2; gt_boxes [B,M,4]; gt_cls [B,M] (present iff 0 <= cls < nc); n_prop int32 [B] or None."""
    for t, name in ((proposals, "proposals"), (gt_boxes, "gt_boxes"), (gt_cls, "gt_cls")):
        _need_device(t, "rcnn_sample", name)
    if proposals.dim() != 3 or proposals.shape[2] != 4:
        raise ValueError(f"rcnn_sample: proposals must be [B,R,4], got {tuple(proposals.shape)}")
    B, R = int(proposals.shape[0]), int(proposals.shape[1])
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4 or tuple(gt_cls.shape) != tuple(gt_boxes.shape[:2]):
        raise ValueError(f"rcnn_sample: gt_boxes must be [B,M,4] and gt_cls [B,M] with B={B}, got {tuple(gt_boxes.shape)} and "
                         f"{tuple(gt_cls.shape)}")
    dev = proposals.device
    pr, gb, gc = _f32(proposals, dev), _f32(gt_boxes, dev), _i32(gt_cls, dev)
    npr = None
    if n_prop is not None:
        _need_device(n_prop, "rcnn_sample", "n_prop")
        if tuple(n_prop.shape) != (B,):
            raise ValueError(f"rcnn_sample: n_prop must be [B], got {tuple(n_prop.shape)}")
        npr = _i32(n_prop, dev)
    cs = c_spec(spec, B=B, R=R, M=int(gb.shape[1]), C=int(nc))
    S = int(cs.S)
    if S < 1:
        raise ValueError("rcnn_sample: S must be >= 1")
    out = Sample(torch.empty((B, S), dtype=torch.int32, device=dev), torch.empty((B, S, 4), dtype=torch.float32, device=dev),
                 torch.empty((B, S), dtype=torch.int32, device=dev), torch.empty((B, S), dtype=torch.int32, device=dev),
                 torch.empty((B, 2), dtype=torch.int32, device=dev))
    call("gsr_rcnn_sample", dev, ctypes.byref(cs), pr.data_ptr(), _ptr(npr), gb.data_ptr(), gc.data_ptr(), out.idx.data_ptr(),
         out.rois.data_ptr(), out.labels.data_ptr(), out.gt_row.data_ptr(), out.counts.data_ptr())
    return out


def _roi_sizes(fn: str, feat_shape, rois: torch.Tensor, counts: Optional[torch.Tensor]):
    if len(feat_shape) != 4:
        raise ValueError(f"{fn}: features must be [B,Cf,Hf,Wf], got {tuple(feat_shape)}")
    B = int(feat_shape[0])
    if rois.dim() != 3 or rois.shape[0] != B or rois.shape[2] != 4:
        raise ValueError(f"{fn}: rois must be [B,S,4] with B={B}, got {tuple(rois.shape)}")
    stride = 0
    if counts is not None:
        if counts.dtype != torch.int32 or not counts.is_contiguous() or counts.shape[0] != B or counts.dim() not in (1, 2):
            raise ValueError(f"{fn}: counts must be a contiguous int32 [B] or [B,k] (column 0 is read)")
        stride = 1 if counts.dim() == 1 else int(counts.shape[1])
    return B, int(rois.shape[1]), stride


def roi_align_forward(features: torch.Tensor, rois: torch.Tensor, counts: Optional[torch.Tensor], spec: RcnnSpec) -> torch.Tensor:
    _need_device(features, "roi_align", "features")
    _need_device(rois, "roi_align", "rois")
    B, S, stride = _roi_sizes("roi_align", features.shape, rois, counts)
    dev = features.device
    f, r = _f32(features, dev), _f32(rois, dev)
    cs = c_spec(spec, B=B, Cf=int(f.shape[1]), Hf=int(f.shape[2]), Wf=int(f.shape[3]), S=S)
    pooled = torch.empty((B, S, int(f.shape[1]), int(cs.PH), int(cs.PW)), dtype=torch.float32, device=dev)
    call("gsr_roi_align", dev, ctypes.byref(cs), f.data_ptr(), r.data_ptr(), _ptr(counts), stride, pooled.data_ptr())
    return pooled


def roi_align_backward(grad_pooled: torch.Tensor, rois: torch.Tensor, counts: Optional[torch.Tensor], feat_shape, spec: RcnnSpec,
                       out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """-> grad_features [B,Cf,Hf,Wf]; `out` with accumulate: added to what `out` holds."""
    _need_device(grad_pooled, "roi_align_backward", "grad_pooled")
    _need_device(rois, "roi_align_backward", "rois")
    B, S, stride = _roi_sizes("roi_align_backward", feat_shape, rois, counts)
    dev = grad_pooled.device
    Cf, Hf, Wf = int(feat_shape[1]), int(feat_shape[2]), int(feat_shape[3])
    cs = c_spec(spec, B=B, Cf=Cf, Hf=Hf, Wf=Wf, S=S)
    if tuple(grad_pooled.shape) != (B, S, Cf, int(cs.PH), int(cs.PW)):
        raise ValueError(f"roi_align_backward: grad_pooled must be {(B, S, Cf, int(cs.PH), int(cs.PW))}, got {tuple(grad_pooled.shape)}")
    g, r = _f32(grad_pooled, dev), _f32(rois, dev)
    if out is None:
        if accumulate:
            raise ValueError("roi_align_backward: accumulate needs `out`")
        out = torch.empty((B, Cf, Hf, Wf), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (B, Cf, Hf, Wf) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("roi_align_backward: `out` must be a contiguous float32 [B,Cf,Hf,Wf] on the gradient's device")
    call("gsr_roi_align_backward", dev, ctypes.byref(cs), r.data_ptr(), _ptr(counts), stride, g.data_ptr(), out.data_ptr(),
         1 if accumulate else 0)
    return out


class _RoiAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, counts, spec):
        pooled = roi_align_forward(features, rois, counts, spec)
        ctx.spec, ctx.feat_shape, ctx.in_dtype = spec, tuple(features.shape), features.dtype
        ctx.rois = rois.detach()
        ctx.counts = counts
        return pooled

    @staticmethod
    def backward(ctx, grad_pooled):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = roi_align_backward(grad_pooled, ctx.rois, ctx.counts, ctx.feat_shape, ctx.spec)
        return g.to(ctx.in_dtype), None, None, None


def roi_align(features: torch.Tensor, rois: torch.Tensor, counts: Optional[torch.Tensor] = None,
              spec: RcnnSpec = RcnnSpec()) -> torch.Tensor:
    """features [B,Cf,Hf,Wf]; rois [B,S,4] in image pixels; counts: None (every row), int32 [B], or a Sample's counts [B,2]
    -> pooled [B,S,Cf,PH,PW], differentiable with respect to the features."""
    if counts is not None:
        _need_device(counts, "roi_align", "counts")
    return _RoiAlign.apply(features, rois, counts, spec)


def _head_sizes(fn: str, scores: torch.Tensor, deltas: torch.Tensor, spec: RcnnSpec) -> Tuple[int, int, int]:
    _need_device(scores, fn, "scores")
    _need_device(deltas, fn, "deltas")
    if scores.dim() != 3 or scores.shape[2] < 2:
        raise ValueError(f"{fn}: scores must be [B,S,C+1] with C >= 1, got {tuple(scores.shape)}")
    B, S, C = int(scores.shape[0]), int(scores.shape[1]), int(scores.shape[2]) - 1
    D = 4 if spec.class_agnostic else 4 * C
    if tuple(deltas.shape) != (B, S, D):
        raise ValueError(f"{fn}: deltas must be {(B, S, D)}, got {tuple(deltas.shape)}")
    return B, S, C


def run_loss(scores: torch.Tensor, deltas: torch.Tensor, rois: torch.Tensor, labels: torch.Tensor, gt_row: torch.Tensor,
             gt_boxes: torch.Tensor, spec: RcnnSpec = RcnnSpec(), want_grad: bool = True):
    """-> (loss float32 [3] = cls, box, total; grad_scores or None; grad_deltas or None)."""
    B, S, C = _head_sizes("rcnn_loss", scores, deltas, spec)
    for t, name in ((rois, "rois"), (labels, "labels"), (gt_row, "gt_row"), (gt_boxes, "gt_boxes")):
        _need_device(t, "rcnn_loss", name)
    if tuple(rois.shape) != (B, S, 4) or tuple(labels.shape) != (B, S) or tuple(gt_row.shape) != (B, S):
        raise ValueError(f"rcnn_loss: rois must be {(B, S, 4)}, labels and gt_row {(B, S)}")
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4:
        raise ValueError(f"rcnn_loss: gt_boxes must be [B,M,4] with B={B}, got {tuple(gt_boxes.shape)}")
    dev = scores.device
    x, d, r, gb = _f32(scores, dev), _f32(deltas, dev), _f32(rois, dev), _f32(gt_boxes, dev)
    lb, gr = _i32(labels, dev), _i32(gt_row, dev)
    cs = c_spec(spec, B=B, M=int(gb.shape[1]), C=C, S=S)
    cs.R, cs.max_det = 0, 0                                    # the workspace of the loss alone
    ws = _ops_common.workspace(workspace_bytes(cs), dev)
    loss = torch.empty((3,), dtype=torch.float32, device=dev)
    gs = torch.empty_like(x) if want_grad else None
    gd = torch.empty_like(d) if want_grad else None
    call("gsr_rcnn_loss", dev, ctypes.byref(cs), x.data_ptr(), d.data_ptr(), r.data_ptr(), lb.data_ptr(), gr.data_ptr(), gb.data_ptr(),
         ws.data_ptr(), ws.numel() * 8, loss.data_ptr(), _ptr(gs), _ptr(gd))
    return loss, gs, gd


class _RcnnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, deltas, rois, labels, gt_row, gt_boxes, spec):
        need = scores.requires_grad or deltas.requires_grad
        loss, gs, gd = run_loss(scores, deltas, rois, labels, gt_row, gt_boxes, spec, want_grad=need)
        ctx.has_grad = need
        ctx.in_dtypes = (scores.dtype, deltas.dtype)
        if need:
            ctx.save_for_backward(gs, gd)
        items = loss[:2].clone()
        ctx.mark_non_differentiable(items)
        return loss[2].clone(), items

    @staticmethod
    def backward(ctx, grad_total, _grad_items):
        if not ctx.has_grad:
            return (None,) * 7
        gs, gd = ctx.saved_tensors
        return ((gs * grad_total).to(ctx.in_dtypes[0]) if ctx.needs_input_grad[0] else None,
                (gd * grad_total).to(ctx.in_dtypes[1]) if ctx.needs_input_grad[1] else None, None, None, None, None, None)


def rcnn_loss(scores: torch.Tensor, deltas: torch.Tensor, rois: torch.Tensor, labels: torch.Tensor, gt_row: torch.Tensor,
              gt_boxes: torch.Tensor, spec: RcnnSpec = RcnnSpec()) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (total, items[2] = cls, box unweighted); total is differentiable with respect to scores and deltas."""
    _head_sizes("rcnn_loss", scores, deltas, spec)
    return _RcnnLoss.apply(scores, deltas, rois, labels, gt_row, gt_boxes, spec)


def postprocess(scores: torch.Tensor, deltas: torch.Tensor, proposals: torch.Tensor, spec: RcnnSpec = RcnnSpec(),
                n_prop: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """scores [B,R,C+1], deltas [B,R,4C] or [B,R,4], proposals [B,R,4] -> (dets float32 [B,max_det,6]: the kept boxes in walk
    order, zero rows beyond; counts int32 [B,2]: kept, candidates)."""
    B, R, C = _head_sizes("rcnn_postprocess", scores, deltas, spec)
    _need_device(proposals, "rcnn_postprocess", "proposals")
    if tuple(proposals.shape) != (B, R, 4):
        raise ValueError(f"rcnn_postprocess: proposals must be {(B, R, 4)}, got {tuple(proposals.shape)}")
    dev = scores.device
    x, d, pr = _f32(scores, dev), _f32(deltas, dev), _f32(proposals, dev)
    npr = None
    if n_prop is not None:
        _need_device(n_prop, "rcnn_postprocess", "n_prop")
        if tuple(n_prop.shape) != (B,):
            raise ValueError(f"rcnn_postprocess: n_prop must be [B], got {tuple(n_prop.shape)}")
        npr = _i32(n_prop, dev)
    cs = c_spec(spec, B=B, R=R, C=C, S=0)
    cs.max_det = min(int(spec.max_det), R)
    ws = _ops_common.workspace(workspace_bytes(cs), dev)
    dets = torch.empty((B, int(cs.max_det), 6), dtype=torch.float32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    call("gsr_rcnn_postprocess", dev, ctypes.byref(cs), x.data_ptr(), d.data_ptr(), pr.data_ptr(), _ptr(npr), ws.data_ptr(),
         ws.numel() * 8, dets.data_ptr(), counts.data_ptr())
    return dets, counts

"""ctypes bindings of the detector output stage (include/gsraster.h, capability bit GSR_CAP_DETECT of gsr_query(3)):

  postprocess  raw head output [B,A,4+has_obj+C] or [B,4+has_obj+C,A] -> (dets [B,max_det,6] x1 y1 x2 y2 score class,
               counts [B,2] kept / above the threshold): score filter, deterministic order, greedy NMS, affine
  nms          the same walk on caller boxes, scores and classes -> (keep [B,max_det] padded with -1, counts [B])
  box_iou      torchvision's box_iou in float32 with every operation rounded on its own
  verdict      the reference's success test for every image of a batch -> (bits int32 [B], best [B,4])

Outputs and the workspace are torch tensors on the input's device; the kernels run on the current stream and nothing
waits for them.  Nothing here is differentiable.  No fallback: tensors must live on a HIP device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

import torch

from . import _load
from . import _ops_common
from ._ops_common import _f32, _i32, _need_device, _ptr, call, capability

GSR_CAP_DETECT = 2
GSR_DET_CLASS_AGNOSTIC = 1
MAX_CANDIDATES = 4096


class DetSpec(NamedTuple):
    """How a head's raw output is read (GsrDetSpec without the sizes, which come from the tensor)."""
    layout: int = 1              # 0: [B,A,K] (YOLOv3/v5), 1: [B,K,A] (YOLOv8/v11); K = 4 + has_obj + C
    has_obj: bool = False
    box_format: int = 0          # 0: (xc, yc, w, h), 1: (x1, y1, x2, y2)
    conf_thr: float = 0.7
    iou_thr: float = 0.45
    max_candidates: int = MAX_CANDIDATES
    max_det: int = 300
    class_agnostic: bool = False
    ox: float = 0.0              # after NMS: x' = (x - ox) * sx, y' = (y - oy) * sy
    oy: float = 0.0
    sx: float = 1.0
    sy: float = 1.0


class _CDetSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("C", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("has_obj", ctypes.c_int32), ("box_format", ctypes.c_int32),
                ("conf_thr", ctypes.c_float), ("iou_thr", ctypes.c_float),
                ("max_candidates", ctypes.c_int32), ("max_det", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("ox", ctypes.c_float), ("oy", ctypes.c_float), ("sx", ctypes.c_float), ("sy", ctypes.c_float)]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """Bit 1 of gsr_query(3): the loaded library has the detector output stage."""
    return capability(3, GSR_CAP_DETECT)


def c_spec(spec: DetSpec, B: int, A: int, C: int) -> _CDetSpec:
    return _CDetSpec(int(B), int(A), int(C), int(spec.layout), 1 if spec.has_obj else 0, int(spec.box_format),
                     float(spec.conf_thr), float(spec.iou_thr), int(spec.max_candidates), int(spec.max_det),
                     GSR_DET_CLASS_AGNOSTIC if spec.class_agnostic else 0, float(spec.ox), float(spec.oy), float(spec.sx),
                     float(spec.sy))


def workspace_bytes(cs: _CDetSpec) -> int:
    return _ops_common.workspace_bytes("gsr_det_workspace_bytes", cs)


def postprocess(raw: torch.Tensor, spec: DetSpec) -> Tuple[torch.Tensor, torch.Tensor]:
    """raw [B,A,K] (spec.layout 0) or [B,K,A] (1), K = 4 + has_obj + C -> (dets [B,max_det,6], counts int32 [B,2])."""
    _need_device(raw, "postprocess", "raw")
    if raw.dim() != 3:
        raise ValueError(f"postprocess: raw must be [B,A,K] or [B,K,A], got {tuple(raw.shape)}")
    x = _f32(raw)
    B = int(x.shape[0])
    A, K = (int(x.shape[1]), int(x.shape[2])) if int(spec.layout) == 0 else (int(x.shape[2]), int(x.shape[1]))
    C = K - 4 - (1 if spec.has_obj else 0)
    if C < 1:
        raise ValueError(f"postprocess: {K} channels leave no class (4 box channels{' and objectness' if spec.has_obj else ''})")
    cs = c_spec(spec, B, A, C)
    ws = _ops_common.workspace(workspace_bytes(cs), x.device)
    dets = torch.empty((B, int(spec.max_det), 6), dtype=torch.float32, device=x.device)
    counts = torch.empty((B, 2), dtype=torch.int32, device=x.device)
    call("gsr_det_postprocess", x.device, ctypes.byref(cs), x.data_ptr(), ws.data_ptr(), ws.numel() * 8, dets.data_ptr(),
         counts.data_ptr())
    return dets, counts


def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_thr: float, max_det: int, classes: Optional[torch.Tensor] = None,
        n_valid: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """boxes [B,n,4] (x1 y1 x2 y2), scores [B,n], classes int [B,n] or None (agnostic), n_valid int [B] or None (n)
    -> (keep int32 [B,max_det]: indices in walk order, -1 padded; counts int32 [B])."""
    _need_device(boxes, "nms", "boxes")
    _need_device(scores, "nms", "scores")
    if boxes.dim() != 3 or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2]):
        raise ValueError(f"nms: boxes must be [B,n,4] and scores [B,n], got {tuple(boxes.shape)} and {tuple(scores.shape)}")
    dev = boxes.device
    bx, sc = _f32(boxes), _f32(scores, dev)
    B, n = int(bx.shape[0]), int(bx.shape[1])
    cl = nv = None
    if classes is not None:
        _need_device(classes, "nms", "classes")
        if tuple(classes.shape) != (B, n):
            raise ValueError(f"nms: classes must be [B,n], got {tuple(classes.shape)}")
        cl = _i32(classes, dev)
    if n_valid is not None:
        _need_device(n_valid, "nms", "n_valid")
        if tuple(n_valid.shape) != (B,):
            raise ValueError(f"nms: n_valid must be [B], got {tuple(n_valid.shape)}")
        nv = _i32(n_valid, dev)
    if n < 1 or n > MAX_CANDIDATES:
        raise ValueError(f"nms: n={n} boxes per image (1..{MAX_CANDIDATES})")
    # the workspace of a spec with A = max_candidates = n (include/gsraster.h)
    cs = _CDetSpec(B, n, 1, 0, 0, 1, 0.0, float(iou_thr), n, 1, 0, 0.0, 0.0, 1.0, 1.0)
    ws = _ops_common.workspace(workspace_bytes(cs), dev)
    keep = torch.empty((B, int(max_det)), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    call("gsr_det_nms", dev, B, n, bx.data_ptr(), sc.data_ptr(), _ptr(cl), _ptr(nv), float(iou_thr), int(max_det), ws.data_ptr(),
         ws.numel() * 8, keep.data_ptr(), counts.data_ptr())
    return keep, counts


def box_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [n,4], b [m,4] (x1 y1 x2 y2) -> iou [n,m] float32."""
    _need_device(a, "box_iou", "a")
    _need_device(b, "box_iou", "b")
    if a.dim() != 2 or a.shape[1] != 4 or b.dim() != 2 or b.shape[1] != 4:
        raise ValueError(f"box_iou: a and b must be [n,4] and [m,4], got {tuple(a.shape)} and {tuple(b.shape)}")
    x, y = _f32(a), _f32(b, a.device)
    out = torch.empty((int(x.shape[0]), int(y.shape[0])), dtype=torch.float32, device=x.device)
    call("gsr_det_box_iou", x.device, x.data_ptr(), int(x.shape[0]), y.data_ptr(), int(y.shape[0]), out.data_ptr())
    return out


def verdict(dets: torch.Tensor, counts: torch.Tensor, gt: Optional[torch.Tensor], target: int, untarget: Optional[int] = None,
            is_targeted: bool = True, iou_match: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """dets [B,max_det,6] and counts [B,2] of `postprocess`, gt [B,4] (x1 y1 x2 y2; None or a NaN row: no gt box)
    -> (bits int32 [B]: 1 success, 2 target_exists, 4 untarget_absent; best [B,4]: iou, score, class, row, -1 if none)."""
    _need_device(dets, "verdict", "dets")
    _need_device(counts, "verdict", "counts")
    if dets.dim() != 3 or dets.shape[2] != 6 or tuple(counts.shape) != (dets.shape[0], 2):
        raise ValueError(f"verdict: dets must be [B,max_det,6] and counts [B,2], got {tuple(dets.shape)} and {tuple(counts.shape)}")
    dev = dets.device
    d = _f32(dets)
    c = _i32(counts, dev)
    B, max_det = int(d.shape[0]), int(d.shape[1])
    g = None
    if gt is not None:
        _need_device(gt, "verdict", "gt")
        if tuple(gt.shape) != (B, 4):
            raise ValueError(f"verdict: gt must be [B,4], got {tuple(gt.shape)}")
        g = _f32(gt, dev)
    bits = torch.empty((B,), dtype=torch.int32, device=dev)
    best = torch.empty((B, 4), dtype=torch.float32, device=dev)
    call("gsr_det_verdict", dev, d.data_ptr(), c.data_ptr(), B, max_det, _ptr(g), int(target), -1 if untarget is None else int(untarget),
         1 if is_targeted else 0, float(iou_match), bits.data_ptr(), best.data_ptr())
    return bits, best

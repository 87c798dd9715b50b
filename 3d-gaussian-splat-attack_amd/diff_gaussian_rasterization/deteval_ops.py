"""ctypes bindings of the detection metrics (include/gsraster.h; no capability bit: present iff the library exports
gsr_deteval_match):

  match       dets [B,D,6] / counts [B,2] of any detector output stage against gt_boxes [B,M,4] / gt_cls [B,M] -> MatchOut:
              the in-image order, the rank within image and class, and COCOeval's match and ignore flags for every area range
              and IoU threshold
  accumulate  the concatenated match outputs of N images -> (precision, scores [T,R,K,A,Mx], recall [T,K,A,Mx], npig [K,A])
  summarize   -> stats float64 [14]: COCOeval.summarize's twelve, then the reference's AP and AR

Everything is float64 arithmetic in a fixed order: the same bits on every run.  Outputs and the workspace are torch tensors on the
input's device; the kernels run on the current stream and nothing waits for them.  No fallback: tensors must live on a HIP
device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Tuple

import torch

from . import _load
from . import _ops_common
from ._ops_common import _f32, _i32, _need_device, _ptr, call

MAX_D, MAX_M, MAX_T, MAX_A, MAX_K, MAX_CAPS, MAX_R, MAX_ROWS = 4096, 256, 10, 4, 65535, 3, 1024, 1 << 20
N_STATS = 14
STAT_NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large",
              "ap_ref", "ar_ref")


class EvalSpec(NamedTuple):
    """GsrDetEvalSpec without D and M, which come from the tensors.  The thresholds and bounds are the caller's doubles."""
    num_classes: int
    iou_thrs: Tuple[float, ...]
    area_ranges: Tuple[Tuple[float, float], ...]
    max_dets: Tuple[int, ...]
    n_rec: int


class _CDetEvalSpec(ctypes.Structure):
    _fields_ = [("K", ctypes.c_int32), ("D", ctypes.c_int32), ("M", ctypes.c_int32), ("T", ctypes.c_int32), ("A", ctypes.c_int32),
                ("n_caps", ctypes.c_int32), ("max_dets", ctypes.c_int32 * MAX_CAPS), ("R", ctypes.c_int32),
                ("iou_thrs", ctypes.c_double * MAX_T), ("area_lo", ctypes.c_double * MAX_A), ("area_hi", ctypes.c_double * MAX_A)]


class MatchOut(NamedTuple):
    dt_order: torch.Tensor      # int32 [B,D]
    dt_rank: torch.Tensor       # int32 [B,D]
    dt_match: torch.Tensor      # int32 [B,A,T,D]
    dt_ignore: torch.Tensor     # uint8 [B,A,T,D]
    gt_ignore: torch.Tensor     # uint8 [B,A,M]
    gt_match: torch.Tensor      # int32 [B,A,T,M]


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """The loaded library has the stage."""
    return hasattr(_load(), "gsr_deteval_match")


def c_spec(spec: EvalSpec, D: int, M: int) -> _CDetEvalSpec:
    if len(spec.iou_thrs) > MAX_T or len(spec.area_ranges) > MAX_A or len(spec.max_dets) > MAX_CAPS:
        raise ValueError(f"deteval: {len(spec.iou_thrs)} IoU thresholds, {len(spec.area_ranges)} area ranges, {len(spec.max_dets)} max_dets "
                         f"(at most {MAX_T}, {MAX_A}, {MAX_CAPS})")
    cs = _CDetEvalSpec(int(spec.num_classes), int(D), int(M), len(spec.iou_thrs), len(spec.area_ranges), len(spec.max_dets))
    for i, c in enumerate(spec.max_dets):
        cs.max_dets[i] = int(c)
    cs.R = int(spec.n_rec)
    for i, v in enumerate(spec.iou_thrs):
        cs.iou_thrs[i] = float(v)
    for i, (lo, hi) in enumerate(spec.area_ranges):
        cs.area_lo[i], cs.area_hi[i] = float(lo), float(hi)
    return cs


def workspace_bytes(cs: _CDetEvalSpec, N: int) -> int:
    lib = _load()
    n = ctypes.c_int64(0)
    rc = lib.gsr_deteval_workspace_bytes(ctypes.byref(cs), int(N), ctypes.byref(n))
    if rc != 0:
        _ops_common._raise(lib, rc)
    return int(n.value)


def _check_dets(fn: str, dets: torch.Tensor) -> None:
    if isinstance(dets, torch.Tensor) and (dets.dim() != 3 or dets.shape[2] != 6):
        raise ValueError(f"{fn}: dets must be [B,D,6], got {tuple(dets.shape)}")
    _need_device(dets, fn, "dets")


def match(dets: torch.Tensor, counts: torch.Tensor, gt_boxes: torch.Tensor, gt_cls: torch.Tensor, spec: EvalSpec) -> MatchOut:
    """dets [B,D,6] (x1 y1 x2 y2 score class), counts [B,2], gt_boxes [B,M,4], gt_cls int [B,M] (a class outside 0..K-1: no row)."""
    _check_dets("match", dets)
    for t, n in ((counts, "counts"), (gt_boxes, "gt_boxes"), (gt_cls, "gt_cls")):
        _need_device(t, "match", n)
    B, D = int(dets.shape[0]), int(dets.shape[1])
    if tuple(counts.shape) != (B, 2) or gt_boxes.dim() != 3 or tuple(gt_boxes.shape[::2]) != (B, 4) or tuple(gt_cls.shape) != tuple(gt_boxes.shape[:2]):
        raise ValueError(f"match: counts must be [B,2], gt_boxes [B,M,4] and gt_cls [B,M], got {tuple(counts.shape)}, {tuple(gt_boxes.shape)} "
                         f"and {tuple(gt_cls.shape)}")
    dev = dets.device
    d, c, gb, gc = _f32(dets), _i32(counts, dev), _f32(gt_boxes, dev), _i32(gt_cls, dev)
    M = int(gb.shape[1])
    cs = c_spec(spec, D, M)
    A, T = cs.A, cs.T
    out = MatchOut(torch.empty((B, D), dtype=torch.int32, device=dev), torch.empty((B, D), dtype=torch.int32, device=dev),
                   torch.empty((B, A, T, D), dtype=torch.int32, device=dev), torch.empty((B, A, T, D), dtype=torch.uint8, device=dev),
                   torch.empty((B, A, M), dtype=torch.uint8, device=dev), torch.empty((B, A, T, M), dtype=torch.int32, device=dev))
    gp = (lambda t: _ptr(t) if M > 0 else None)
    call("gsr_deteval_match", dev, ctypes.byref(cs), B, d.data_ptr(), c.data_ptr(), gp(gb), gp(gc), out.dt_order.data_ptr(),
         out.dt_rank.data_ptr(), out.dt_match.data_ptr(), out.dt_ignore.data_ptr(), gp(out.gt_ignore), gp(out.gt_match))
    return out


def accumulate(dets: torch.Tensor, m: MatchOut, gt_cls: torch.Tensor, rec_thrs: torch.Tensor, spec: EvalSpec):
    """dets [N,D,6] and the match outputs of the same N images, gt_cls int [N,M], rec_thrs float64 [R] on the device
    -> (precision [T,R,K,A,Mx], scores [T,R,K,A,Mx], recall [T,K,A,Mx] float64, npig int32 [K,A])."""
    _check_dets("accumulate", dets)
    for t, n in ((gt_cls, "gt_cls"), (rec_thrs, "rec_thrs")) + tuple(zip(m, MatchOut._fields)):
        _need_device(t, "accumulate", n)
    dev = dets.device
    N, D = int(dets.shape[0]), int(dets.shape[1])
    if rec_thrs.dtype != torch.float64 or rec_thrs.dim() != 1 or int(rec_thrs.shape[0]) != int(spec.n_rec):
        raise ValueError(f"accumulate: rec_thrs must be float64 [{spec.n_rec}], got {rec_thrs.dtype} {tuple(rec_thrs.shape)}")
    if gt_cls.dim() != 2 or int(gt_cls.shape[0]) != N:
        raise ValueError(f"accumulate: gt_cls must be [N,M] with N={N}, got {tuple(gt_cls.shape)}")
    M = int(gt_cls.shape[1])
    cs = c_spec(spec, D, M)
    A, T, K, R, Mx = cs.A, cs.T, cs.K, cs.R, cs.n_caps
    want = dict(dt_order=(N, D), dt_rank=(N, D), dt_match=(N, A, T, D), dt_ignore=(N, A, T, D), gt_ignore=(N, A, M), gt_match=(N, A, T, M))
    for name, t in zip(MatchOut._fields, m):
        if tuple(t.shape) != want[name] or t.dtype != (torch.uint8 if name.endswith("ignore") else torch.int32):
            raise ValueError(f"accumulate: {name} must be {t.dtype} {want[name]}, got {tuple(t.shape)}")
    d, gc, rt = _f32(dets), _i32(gt_cls, dev), rec_thrs.contiguous()
    mm = [t.contiguous() for t in m]
    ws = _ops_common.workspace(workspace_bytes(cs, N), dev)
    precision = torch.empty((T, R, K, A, Mx), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, K, A, Mx), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, Mx), dtype=torch.float64, device=dev)
    npig = torch.empty((K, A), dtype=torch.int32, device=dev)
    gp = (lambda t: _ptr(t) if M > 0 else None)
    call("gsr_deteval_accumulate", dev, ctypes.byref(cs), N, d.data_ptr(), mm[0].data_ptr(), mm[1].data_ptr(), mm[2].data_ptr(),
         mm[3].data_ptr(), gp(gc), gp(mm[4]), rt.data_ptr(), ws.data_ptr(), ws.numel() * 8, precision.data_ptr(), scores.data_ptr(),
         recall.data_ptr(), npig.data_ptr())
    return precision, scores, recall, npig


def summarize(precision: torch.Tensor, recall: torch.Tensor, spec: EvalSpec) -> torch.Tensor:
    """precision [T,R,K,A,Mx], recall [T,K,A,Mx] (float64, device) -> stats float64 [14] in the order of STAT_NAMES."""
    _need_device(precision, "summarize", "precision")
    _need_device(recall, "summarize", "recall")
    cs = c_spec(spec, 1, 0)
    cs.D = max(int(c) for c in spec.max_dets)          # (the summary reads neither D nor M; the caps must pass the spec check)
    shape = (cs.T, cs.R, cs.K, cs.A, cs.n_caps)
    if precision.dtype != torch.float64 or recall.dtype != torch.float64 or tuple(precision.shape) != shape \
            or tuple(recall.shape) != shape[:1] + shape[2:]:
        raise ValueError(f"summarize: precision must be float64 {shape} and recall {shape[:1] + shape[2:]}, got {tuple(precision.shape)} and "
                         f"{tuple(recall.shape)}")
    p, r = precision.contiguous(), recall.contiguous()
    stats = torch.empty((N_STATS,), dtype=torch.float64, device=p.device)
    call("gsr_deteval_summarize", p.device, ctypes.byref(cs), p.data_ptr(), r.data_ptr(), stats.data_ptr())
    return stats

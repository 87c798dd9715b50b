"""ctypes binding of the RPN proposal stage (include/gsraster.h, capability bit GSR_CAP_RPN of gsr_query(5)): from the RPN
head's objectness logits and anchor deltas to the proposals the two-stage stage samples from.

  select    one level: logits [B,A,Hf,Wf], deltas [B,4A,Hf,Wf], cell_anchors [A,4] -> that level's range of the candidate
            slots (cand_boxes [B,N,4], cand_scores [B,N], cand_level [B,N]) written in place: one C call
  nms       the candidate slots -> Proposals(boxes [B,post_topk,4], scores [B,post_topk], keep [B,post_topk], counts [B])
  propose   a list of levels chained through cand_offset, then nms

Outputs and the workspace are torch tensors on the inputs' device; the kernels run on the current stream and nothing waits
for them.  No fallback: tensors must live on a HIP device; CPU tensors raise.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence, Tuple

import torch

from . import _load
from . import _ops_common
from ._ops_common import _f32, _i32, _need_device, call, capability

GSR_CAP_RPN = 32
MAX_SLOTS = 16384
MAX_POST = 4096


class RpnSpec(NamedTuple):
    """GsrRpnSpec without the sizes, the level's own members and the slot layout, which come from the tensors and the
    call.  The defaults are Detectron2's RPN in training mode, as the reference runs it."""
    img_w: float = 1.0
    img_h: float = 1.0
    min_size: float = 0.0
    pre_topk: int = 12000
    post_topk: int = 2000
    iou_thr: float = 0.7


class _CRpnSpec(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("Hf", ctypes.c_int32), ("Wf", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("shift0", ctypes.c_float), ("img_w", ctypes.c_float), ("img_h", ctypes.c_float),
                ("min_size", ctypes.c_float), ("pre_topk", ctypes.c_int32), ("level", ctypes.c_int32),
                ("cand_offset", ctypes.c_int32), ("N", ctypes.c_int32), ("post_topk", ctypes.c_int32),
                ("iou_thr", ctypes.c_float), ("flags", ctypes.c_uint32)]


class Level(NamedTuple):
    """One feature level of `propose`: the head's outputs on it, its cell anchors [A,4], its stride in pixels and
    Detectron2's anchor offset (0 unless the generator was built with one)."""
    logits: torch.Tensor
    deltas: torch.Tensor
    cell_anchors: torch.Tensor
    stride: int
    offset: float = 0.0


class Proposals(NamedTuple):
    """What gsr_rpn_nms writes: boxes [B,post_topk,4] and scores [B,post_topk] in walk order, zeros beyond the count; keep
    int32 [B,post_topk]: the kept candidate slots, -1 beyond; counts int32 [B]."""
    boxes: torch.Tensor
    scores: torch.Tensor
    keep: torch.Tensor
    counts: torch.Tensor


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def available() -> bool:
    """Bit 5 of gsr_query(5), the item that holds every capability bit (items 3 and 4 are closed at 15 and 31): the loaded
    library has the RPN proposal stage.  A library without item 5 refuses it: no stage."""
    return capability(5, GSR_CAP_RPN)


def c_spec(spec: RpnSpec, B: int = 1, A: int = 1, Hf: int = 1, Wf: int = 1, stride: int = 1, shift0: float = 0.0, level: int = 0,
           cand_offset: int = 0, N: int = 1) -> _CRpnSpec:
    return _CRpnSpec(int(B), int(A), int(Hf), int(Wf), int(stride), float(shift0), float(spec.img_w), float(spec.img_h),
                     float(spec.min_size), int(spec.pre_topk), int(level), int(cand_offset), int(N), int(spec.post_topk),
                     float(spec.iou_thr), 0)


def workspace_bytes(cs: _CRpnSpec) -> int:
    return _ops_common.workspace_bytes("gsr_rpn_workspace_bytes", cs)


def level_slots(logits_shape, pre_topk: int) -> int:
    """The slots a level fills: min(pre_topk, A * Hf * Wf)."""
    return min(int(pre_topk), int(logits_shape[1]) * int(logits_shape[2]) * int(logits_shape[3]))


def new_candidates(B: int, N: int, dev) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Candidate arrays for `select` to fill: no slot takes part in `nms` until a level has written it."""
    return (torch.zeros((B, N, 4), dtype=torch.float32, device=dev), torch.zeros((B, N), dtype=torch.float32, device=dev),
            torch.full((B, N), -1, dtype=torch.int32, device=dev))


def select(logits: torch.Tensor, deltas: torch.Tensor, cell_anchors: torch.Tensor, stride: int, spec: RpnSpec,
           cand: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], level: int = 0, cand_offset: int = 0, offset: float = 0.0) -> int:
    """Fills slots cand_offset .. cand_offset + n - 1 of cand = (cand_boxes [B,N,4], cand_scores [B,N], cand_level [B,N])
    in place -> n, the slots of this level."""
    for t, name in ((logits, "logits"), (deltas, "deltas"), (cell_anchors, "cell_anchors")) + tuple(zip(cand, ("cand_boxes", "cand_scores", "cand_level"))):
        _need_device(t, "rpn_select", name)
    if logits.dim() != 4:
        raise ValueError(f"rpn_select: logits must be [B,A,Hf,Wf], got {tuple(logits.shape)}")
    B, A, Hf, Wf = (int(v) for v in logits.shape)
    if tuple(deltas.shape) != (B, 4 * A, Hf, Wf):
        raise ValueError(f"rpn_select: deltas must be {(B, 4 * A, Hf, Wf)}, got {tuple(deltas.shape)}")
    if tuple(cell_anchors.shape) != (A, 4):
        raise ValueError(f"rpn_select: cell_anchors must be {(A, 4)}, got {tuple(cell_anchors.shape)}")
    cb, csc, cl = cand
    N = int(csc.shape[1]) if csc.dim() == 2 else -1
    if (tuple(cb.shape) != (B, N, 4) or tuple(csc.shape) != (B, N) or tuple(cl.shape) != (B, N) or cb.dtype != torch.float32
            or csc.dtype != torch.float32 or cl.dtype != torch.int32 or not (cb.is_contiguous() and csc.is_contiguous() and cl.is_contiguous())):
        raise ValueError("rpn_select: cand must be contiguous (float32 [B,N,4], float32 [B,N], int32 [B,N])")
    dev = logits.device
    lg, dl, ca = _f32(logits, dev), _f32(deltas, dev), _f32(cell_anchors, dev)
    cs = c_spec(spec, B=B, A=A, Hf=Hf, Wf=Wf, stride=stride, shift0=float(offset) * int(stride), level=level, cand_offset=cand_offset, N=N)
    call("gsr_rpn_select", dev, ctypes.byref(cs), lg.data_ptr(), dl.data_ptr(), ca.data_ptr(), cb.data_ptr(), csc.data_ptr(), cl.data_ptr())
    return level_slots(logits.shape, spec.pre_topk)


def nms(cand_boxes: torch.Tensor, cand_scores: torch.Tensor, cand_level: torch.Tensor, spec: RpnSpec) -> Proposals:
    """cand_boxes [B,N,4], cand_scores [B,N], cand_level [B,N] (negative: the slot does not take part) -> Proposals; the rows
    per image are min(spec.post_topk, N, 4096)."""
    for t, name in ((cand_boxes, "cand_boxes"), (cand_scores, "cand_scores"), (cand_level, "cand_level")):
        _need_device(t, "rpn_nms", name)
    if cand_scores.dim() != 2 or tuple(cand_boxes.shape) != tuple(cand_scores.shape) + (4,) or tuple(cand_level.shape) != tuple(cand_scores.shape):
        raise ValueError(f"rpn_nms: cand_boxes must be [B,N,4], cand_scores and cand_level [B,N], got {tuple(cand_boxes.shape)}, "
                         f"{tuple(cand_scores.shape)} and {tuple(cand_level.shape)}")
    B, N = int(cand_scores.shape[0]), int(cand_scores.shape[1])
    dev = cand_scores.device
    cb, csc, cl = _f32(cand_boxes, dev), _f32(cand_scores, dev), _i32(cand_level, dev)
    post = min(int(spec.post_topk), N, MAX_POST)
    cs = c_spec(spec._replace(post_topk=post), B=B, N=N)
    ws = _ops_common.workspace(workspace_bytes(cs), dev)
    out = Proposals(torch.empty((B, post, 4), dtype=torch.float32, device=dev), torch.empty((B, post), dtype=torch.float32, device=dev),
                    torch.empty((B, post), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
    call("gsr_rpn_nms", dev, ctypes.byref(cs), cb.data_ptr(), csc.data_ptr(), cl.data_ptr(), ws.data_ptr(), ws.numel() * 8,
         out.boxes.data_ptr(), out.scores.data_ptr(), out.keep.data_ptr(), out.counts.data_ptr())
    return out


def propose(levels: Sequence[Level], spec: RpnSpec, return_candidates: bool = False):
    """find_top_rpn_proposals over the levels: level l fills the slots behind level l - 1's, then one NMS walk over all of
    them -> Proposals (with return_candidates: (Proposals, (cand_boxes, cand_scores, cand_level)))."""
    if len(levels) < 1:
        raise ValueError("rpn_propose: at least one level")
    levels = [Level(*lv) for lv in levels]
    for lv in levels:
        _need_device(lv.logits, "rpn_propose", "logits")
        if lv.logits.dim() != 4 or lv.logits.shape[0] != levels[0].logits.shape[0]:
            raise ValueError("rpn_propose: every level's logits must be [B,A,Hf,Wf] with the same B")
    sizes = [level_slots(lv.logits.shape, spec.pre_topk) for lv in levels]
    N = sum(sizes)
    if N > MAX_SLOTS:
        raise ValueError(f"rpn_propose: {N} candidate slots over the levels (at most {MAX_SLOTS})")
    cand = new_candidates(int(levels[0].logits.shape[0]), N, levels[0].logits.device)
    off = 0
    for l, (lv, n) in enumerate(zip(levels, sizes)):
        select(lv.logits, lv.deltas, lv.cell_anchors, lv.stride, spec, cand, level=l, cand_offset=off, offset=lv.offset)
        off += n
    out = nms(*cand, spec)
    return (out, cand) if return_candidates else out

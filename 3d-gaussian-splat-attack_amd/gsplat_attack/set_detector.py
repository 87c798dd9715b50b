"""Both sides of a set-prediction (DETR-style) detector, on the set-prediction stage's HIP kernels
(diff_gaussian_rasterization.setdet_ops).  Such a head emits Q queries per image, each with C + 1 logits whose last entry
is "no object" and a box (cx, cy, w, h) normalised to the image.

The objective the reference's DETR wrapper descends on (detectors/detr_detector.py:98-115) is DETR's set criterion: a
one-to-one match of the ground-truth rows to queries, then weighted cross-entropy, L1 and GIoU.  Here the match, the loss
and its gradient are computed on the device with a fixed result, so that a PGD step is bitwise reproducible from the loss
back to the Gaussian parameters and no step waits for a host solve.  Its success test (:186-243) is a softmax, a threshold
and an IoU against the view's box, without NMS.  include/gsraster.h holds the formulas; INTEGRATION.md lists the stated
deviations.

  SetDetectorLoss    .loss(logits, boxes, gt_boxes, gt_cls) -> (total, items[3] = ce, l1, giou); .matching(...) -> (match, tgt)
  SetDetectorOutput  .detect(logits, boxes) -> (dets, counts); .verdicts(logits, boxes, gt_bboxes, target, ...) on gsr_det_verdict
  make_set_loss_fn   renders -> detector_input -> detector_head -> SetDetectorLoss as pgd_attack's loss_fn; it takes the global
                     view indices of the renders (loss_fn.takes_view_index) to pick their boxes
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple, Union

import torch

from diff_gaussian_rasterization import setdet_ops
from diff_gaussian_rasterization.setdet_ops import SetDetSpec

from ._views import ViewRows, gt_rows, verdict_of


def _frame(frame) -> Tuple[float, float]:
    w, h = float(frame[0]), float(frame[1])
    if not (w > 0 and h > 0):
        raise ValueError("frame must be (img_w, img_h) with both > 0")
    return w, h


def _head_output(out) -> Tuple[torch.Tensor, torch.Tensor]:
    """A DETR head returns {"pred_logits", "pred_boxes"}; a pair (logits, boxes) is taken as it is."""
    if isinstance(out, dict):
        return out["pred_logits"], out["pred_boxes"]
    logits, boxes = out
    return logits, boxes


class SetDetectorLoss:
    """nc classes (the head emits nc + 1 logits per query); frame = (img_w, img_h): the pixel frame the ground-truth boxes
    are given in, x1 y1 x2 y2 -- the stage normalises them; the cost and loss weights are DETR's."""

    def __init__(self, nc: int, frame: Tuple[float, float], cost_class: float = 1.0, cost_l1: float = 5.0, cost_giou: float = 2.0,
                 ce: float = 1.0, l1: float = 5.0, giou: float = 2.0, eos_coef: float = 0.1):
        if not 1 <= nc <= setdet_ops.MAX_CLASSES:
            raise ValueError(f"SetDetectorLoss: nc must be 1..{setdet_ops.MAX_CLASSES}")
        vals = (cost_class, cost_l1, cost_giou, ce, l1, giou, eos_coef)
        if not all(float(v) >= 0 and float(v) < float("inf") for v in vals):
            raise ValueError("SetDetectorLoss: the cost and loss weights must be finite and >= 0")
        w, h = _frame(frame)
        self.nc = int(nc)
        self.spec = SetDetSpec(w, h, *(float(v) for v in vals))

    def _gt(self, gt_boxes, gt_cls, device) -> Tuple[torch.Tensor, torch.Tensor]:
        return gt_rows(gt_boxes, gt_cls, device)

    def _check(self, logits: torch.Tensor) -> None:
        if logits.dim() != 3 or logits.shape[2] != self.nc + 1:
            raise ValueError(f"SetDetectorLoss: logits must be [B,Q,{self.nc + 1}], got {tuple(logits.shape)}")

    def loss(self, logits: torch.Tensor, boxes: torch.Tensor, gt_boxes, gt_cls) -> Tuple[torch.Tensor, torch.Tensor]:
        """logits [B,Q,nc+1]; boxes [B,Q,4] normalised cx cy w h; gt_boxes [B,M,4] (or [B,4]: one row per image) x1 y1 x2 y2 in
        pixels of the frame; gt_cls [B,M] (or [B]), negative: absent -> (total, items[3] = ce, l1, giou unweighted)."""
        self._check(logits)
        gb, gc = self._gt(gt_boxes, gt_cls, logits.device)
        return setdet_ops.setdet_loss(logits, boxes, gb, gc, self.spec)

    def matching(self, logits: torch.Tensor, boxes: torch.Tensor, gt_boxes, gt_cls) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (match int32 [B,M]: the query of every row, -1 for an absent one; tgt int32 [B,Q]: the row of every query, -1
        for an unmatched one)."""
        self._check(logits)
        gb, gc = self._gt(gt_boxes, gt_cls, logits.device)
        _, _, _, match, tgt = setdet_ops.run(logits, boxes, gb, gc, self.spec, want_grad=False, want_matching=True)
        return match, tgt


class SetDetectorOutput:
    """frame = (img_w, img_h): the pixel frame the detections come out in (the reference: the render's size); conf: the
    score a query must exceed (the reference: 0.7); max_det: rows per image (default: every query)."""

    def __init__(self, frame: Tuple[float, float], conf: float = 0.7, max_det: Optional[int] = None):
        if max_det is not None and not 1 <= max_det <= setdet_ops.MAX_QUERIES:
            raise ValueError(f"SetDetectorOutput: max_det must be 1..{setdet_ops.MAX_QUERIES}")
        w, h = _frame(frame)
        self.spec = SetDetSpec(img_w=w, img_h=h, conf_thr=float(conf), max_det=None if max_det is None else int(max_det))

    def detect(self, logits: torch.Tensor, boxes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (dets [B,max_det,6]: x1 y1 x2 y2 score class of the kept queries in query order, zero rows beyond; counts int32
        [B,2]: kept, above the threshold), both on the logits' device."""
        return setdet_ops.postprocess(logits, boxes, self.spec)

    def verdicts(self, logits: torch.Tensor, boxes: torch.Tensor, gt_bboxes: Optional[torch.Tensor], target: int,
                 untarget: Optional[int] = None, is_targeted: bool = True, iou_match: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
        """gt_bboxes [B,4] (x1 y1 x2 y2 in the frame; None or a NaN row: no box for that view)
        -> (flags int32 [B] on the device: bit 0 success, bit 1 target_exists, bit 2 untarget_absent;
            best [B,4]: iou, score, class, row of the detection closest to the gt box, -1 where there is none)."""
        return verdict_of(*self.detect(logits, boxes), gt_bboxes, target, untarget, is_targeted, iou_match)


def make_set_loss_fn(detector_head: Callable, detector_input: Optional[Callable], detector_loss: SetDetectorLoss, gt_bboxes,
                     target: Union[int, Sequence[int]]) -> Callable:
    """-> loss_fn(renders [B,3,H,W], idx=None) -> total, for pgd_attack(loss_fn=...).  detector_head returns
    {"pred_logits", "pred_boxes"} or (logits, boxes); gt_bboxes [V,4]: every view's box in detector_loss's frame; target: the
    class the loss pulls towards, one int or one per view; idx: the views the renders show (default 0..B-1).  The loss of a
    batch is normalised over the batch, as the criterion does; pgd_attack(batch_loss=True) calls it once per step."""
    views = ViewRows(gt_bboxes, target)

    def loss_fn(renders: torch.Tensor, idx: Optional[Sequence[int]] = None) -> torch.Tensor:
        x, gt, cls = views(renders, idx)
        logits, boxes = _head_output(detector_head(detector_input(x) if detector_input is not None else x))
        return detector_loss.loss(logits, boxes, gt, cls)[0]

    loss_fn.takes_view_index = True
    return loss_fn

"""The objective the reference's YOLO wrappers descend on, on the detector loss stage's HIP kernels
(diff_gaussian_rasterization.detloss_ops): the anchor-free detection loss of the head's raw training output against the
one ground-truth box and target class of every view -- task-aligned assigner, BCE, CIoU and DFL, returned as
box*7.5 + cls*0.5 + dfl*1.5 -- with a deterministic gradient, so that a PGD step is bitwise reproducible from the loss
back to the Gaussian parameters.

The reference ends infer() of all four YOLO wrappers this way (detectors/yolov8_detector.py:115-156): letterbox the
render, scale and shift the view's box into the letterboxed frame (:122-127), call the ultralytics DetectionModel in
training mode.  include/gsraster.h holds the formulas; INTEGRATION.md lists the stated deviations.

  DetectorLoss   .loss(pred or list of feature maps, gt_boxes, gt_cls) -> (total, items[3]); .assignment(...) -> (tgt, ts);
                 .to_letterbox(scale, pad_left, pad_top) maps render-frame boxes into the network's frame
  make_loss_fn   renders -> detector_input -> detector_head -> DetectorLoss as pgd_attack's loss_fn; it takes the global
                 view indices of the renders (loss_fn.takes_view_index) to pick their boxes
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

from diff_gaussian_rasterization import detloss_ops
from diff_gaussian_rasterization.detloss_ops import DetLossSpec

from ._views import ViewRows, gt_rows

Levels = List[Tuple[int, int, float]]


class DetectorLoss:
    """nc classes; strides of the head's levels (a flat pred [B,64+nc,A] also needs input_hw, the network input's size,
    to derive the level table; a list of feature maps [B,64+nc,h_i,w_i] carries it in its shapes)."""

    def __init__(self, nc: int, strides: Sequence[float] = (8, 16, 32), input_hw: Optional[Tuple[int, int]] = None, topk: int = 10,
                 alpha: float = 0.5, beta: float = 6.0, box: float = 7.5, cls: float = 0.5, dfl: float = 1.5):
        if nc < 1:
            raise ValueError("DetectorLoss: nc must be >= 1")
        if not 1 <= len(strides) <= detloss_ops.MAX_LEVELS:
            raise ValueError(f"DetectorLoss: 1..{detloss_ops.MAX_LEVELS} strides")
        if not 1 <= topk <= detloss_ops.MAX_TOPK:
            raise ValueError(f"DetectorLoss: topk must be 1..{detloss_ops.MAX_TOPK}")
        self.nc = int(nc)
        self.strides = tuple(float(s) for s in strides)
        self.input_hw = None if input_hw is None else (int(input_hw[0]), int(input_hw[1]))
        self.spec = DetLossSpec(int(topk), float(alpha), float(beta), float(box), float(cls), float(dfl))
        self.affine = (1.0, 0.0, 0.0)              # gt' = gt * scale + (pad_left, pad_top)

    def to_letterbox(self, scale: float, pad_left: float, pad_top: float) -> "DetectorLoss":
        """detector_input.letterbox's (scale, pad_left, pad_top): boxes given in the render's frame are scaled and shifted
        into the letterboxed one (yolov8_detector.py:122-127)."""
        new = object.__new__(DetectorLoss)
        new.__dict__.update(self.__dict__)
        new.affine = (float(scale), float(pad_left), float(pad_top))
        return new

    def _flatten(self, pred) -> Tuple[torch.Tensor, Levels]:
        if isinstance(pred, (list, tuple)):
            if len(pred) != len(self.strides):
                raise ValueError(f"DetectorLoss: {len(pred)} feature maps for {len(self.strides)} strides")
            levels = [(int(f.shape[2]), int(f.shape[3]), s) for f, s in zip(pred, self.strides)]
            flat = torch.cat([f.reshape(f.shape[0], f.shape[1], -1) for f in pred], dim=2)
        else:
            if self.input_hw is None:
                raise ValueError("DetectorLoss: a flat pred needs input_hw to derive the levels")
            levels = [(int(self.input_hw[0] // s), int(self.input_hw[1] // s), s) for s in self.strides]
            flat = pred
        if flat.dim() != 3 or flat.shape[1] != 64 + self.nc:
            raise ValueError(f"DetectorLoss: pred must have {64 + self.nc} channels, got {tuple(flat.shape)}")
        return flat, levels

    def _gt(self, gt_boxes, gt_cls, device) -> Tuple[torch.Tensor, torch.Tensor]:
        return gt_rows(gt_boxes, gt_cls, device, self.affine)

    def loss(self, pred: Union[torch.Tensor, Sequence[torch.Tensor]], gt_boxes, gt_cls) -> Tuple[torch.Tensor, torch.Tensor]:
        """pred [B,64+nc,A] or the head's feature maps; gt_boxes [B,M,4] (or [B,4]: one row per image) x1 y1 x2 y2; gt_cls
        [B,M] (or [B]), negative: absent -> (total, items[3] = box, cls, dfl unweighted)."""
        flat, levels = self._flatten(pred)
        gb, gc = self._gt(gt_boxes, gt_cls, flat.device)
        return detloss_ops.detloss(flat, levels, gb, gc, self.spec)

    def assignment(self, pred, gt_boxes, gt_cls) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (tgt int32 [B,A]: the gt row of every anchor, -1 for background; ts float32 [B,A]: its target score)."""
        flat, levels = self._flatten(pred)
        gb, gc = self._gt(gt_boxes, gt_cls, flat.device)
        _, _, tgt, ts = detloss_ops.run(flat, levels, gb, gc, self.spec, want_grad=False, want_assignment=True)
        return tgt, ts


def make_loss_fn(detector_head: Callable, detector_input: Optional[Callable], detector_loss: DetectorLoss, gt_bboxes,
                 target: Union[int, Sequence[int]]) -> Callable:
    """-> loss_fn(renders [B,3,H,W], idx=None) -> total, for pgd_attack(loss_fn=...).  gt_bboxes [V,4]: every view's box in
    the frame detector_loss expects (use detector_loss.to_letterbox for boxes in the render's frame); target: the class
    the loss pulls towards, one int or one per view; idx: the views the renders show (default 0..B-1).  The loss of a
    batch is normalised over the batch, as the library does; pgd_attack(batch_loss=True) calls it once per step."""
    views = ViewRows(gt_bboxes, target)

    def loss_fn(renders: torch.Tensor, idx: Optional[Sequence[int]] = None) -> torch.Tensor:
        x, gt, cls = views(renders, idx)
        feats = detector_head(detector_input(x) if detector_input is not None else x)
        return detector_loss.loss(feats, gt, cls)[0]

    loss_fn.takes_view_index = True
    return loss_fn

"""What sits behind a detector's network, on the detector output stage's HIP kernels
(diff_gaussian_rasterization.detect_ops): score filter, deterministic order, greedy NMS, the affine back to the render
frame and the reference's success test, for a whole batch of views without a round trip to the host per view.

The reference does this per view in host Python (predict_and_save of detectors/yolov5_detector.py:107-245 and its
siblings): ultralytics' NMS inside the YOLO wrapper (:127-129), boxes scaled back to the render (:122-125, :155-158),
torchvision's box_iou against the ground-truth box and an argmax (:175-187), the class tests without one (:189-190) and
the verdict (:239-245).  Stated deviations: classes are compared as integers instead of ultralytics' class-offset trick
(equal up to the rounding of the shifted coordinates); a NaN score is dropped and a NaN IoU suppresses and matches
nothing; one label per anchor (no multi_label mode).

  DetectorOutput   how one head's raw output is read; .detections(raw) and .verdict(raw, gt_bboxes, target, ...)
  batch_success    renders [B,3,H,W] -> list of B bools with ONE device-to-host copy
  make_success_fn  the same as pgd_attack's success_fn(image, idx) -> bool
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from diff_gaussian_rasterization import detect_ops
from diff_gaussian_rasterization.detect_ops import DetSpec

from ._views import ViewRows, verdict_of


class DetectorOutput:
    """layout 0: raw [B,A,4+has_obj+C] (YOLOv3/v5), 1: raw [B,4+has_obj+C,A] (YOLOv8/v11); box_format 0: (xc, yc, w, h),
    1: (x1, y1, x2, y2); conf / iou / max_det as ultralytics names them.  The boxes stay in the network's frame unless
    from_letterbox / from_resize set the affine back to the render."""

    def __init__(self, layout: int, has_obj: bool, box_format: int, conf: float = 0.7, iou: float = 0.45, max_det: int = 300,
                 max_candidates: int = detect_ops.MAX_CANDIDATES, class_agnostic: bool = False):
        if layout not in (0, 1) or box_format not in (0, 1):
            raise ValueError("DetectorOutput: layout and box_format are 0 or 1")
        if not 1 <= max_candidates <= detect_ops.MAX_CANDIDATES or not 1 <= max_det <= max_candidates:
            raise ValueError(f"DetectorOutput: 1 <= max_det <= max_candidates <= {detect_ops.MAX_CANDIDATES}")
        self.spec = DetSpec(int(layout), bool(has_obj), int(box_format), float(conf), float(iou), int(max_candidates),
                            int(max_det), bool(class_agnostic))

    def _with_affine(self, ox: float, oy: float, sx: float, sy: float) -> "DetectorOutput":
        new = object.__new__(DetectorOutput)
        new.spec = self.spec._replace(ox=float(ox), oy=float(oy), sx=float(sx), sy=float(sy))
        return new

    def from_letterbox(self, scale: float, pad_left: int, pad_top: int) -> "DetectorOutput":
        """The inverse of detector_input.letterbox (its scale, pad_left, pad_top): x' = (x - pad_left) / scale."""
        return self._with_affine(pad_left, pad_top, 1.0 / scale, 1.0 / scale)

    def from_resize(self, orig_hw: Tuple[int, int], resized_hw: Tuple[int, int]) -> "DetectorOutput":
        """yolov5_detector.py:122-125: x' = x * (orig_w / resized_w), y' = y * (orig_h / resized_h)."""
        return self._with_affine(0.0, 0.0, orig_hw[1] / resized_hw[1], orig_hw[0] / resized_hw[0])

    def detections(self, raw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (dets [B,max_det,6]: x1 y1 x2 y2 score class, zero rows beyond the kept ones; counts int32 [B,2]: kept,
        above the threshold), both on raw's device."""
        return detect_ops.postprocess(raw, self.spec)

    def verdict(self, raw: torch.Tensor, gt_bboxes: Optional[torch.Tensor], target: int, untarget: Optional[int] = None,
                is_targeted: bool = True, iou_match: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
        """gt_bboxes [B,4] (x1 y1 x2 y2 in the frame the affine maps to; None or a NaN row: no box for that view)
        -> (flags int32 [B] on the device: bit 0 success, bit 1 target_exists, bit 2 untarget_absent;
            best [B,4]: iou, score, class, row of the detection closest to the gt box, -1 where there is none)."""
        return verdict_of(*self.detections(raw), gt_bboxes, target, untarget, is_targeted, iou_match)


def batch_success(images: torch.Tensor, detector_head: Callable[[torch.Tensor], torch.Tensor], detector_input: Callable,
                  detector_output: DetectorOutput, gt_bboxes, target: int, untarget: Optional[int] = None,
                  is_targeted: bool = True, iou_match: float = 0.5, idx: Optional[Sequence[int]] = None) -> List[bool]:
    """images [B,3,H,W] -> detector_input -> detector_head (raw output) -> detector_output.verdict; the B success bits
    come back in one device-to-host copy.  gt_bboxes: [V,4] or None; idx: the views the images show (default 0..B-1)."""
    with torch.no_grad():
        x, gt, _ = ViewRows(gt_bboxes)(images, idx)
        raw = detector_head(detector_input(x) if detector_input is not None else x)
        flags, _ = detector_output.verdict(raw, gt, target, untarget, is_targeted, iou_match)
        return [bool(v & 1) for v in flags.cpu().tolist()]


def make_success_fn(detector_head: Callable[[torch.Tensor], torch.Tensor], detector_input: Callable,
                    detector_output: DetectorOutput, gt_bboxes, target: int, untarget: Optional[int] = None,
                    is_targeted: bool = True, iou_match: float = 0.5) -> Callable[[torch.Tensor, int], bool]:
    """-> success_fn(image [3,H,W], view index) -> bool for pgd_attack / run_attack; success_fn.batch_success(images,
    idx=None) -> list[bool] checks a whole batch with one copy."""
    def batch(images: torch.Tensor, idx: Optional[Sequence[int]] = None) -> List[bool]:
        return batch_success(images, detector_head, detector_input, detector_output, gt_bboxes, target, untarget, is_targeted,
                             iou_match, idx)

    def success_fn(image: torch.Tensor, idx: int) -> bool:
        return batch(image[None], [idx])[0]

    success_fn.batch_success = batch
    return success_fn

"""The steps every detector stage's adapters share, one copy each: the ground-truth rows a loss kernel is given
(gt_rows), which views a loss_fn / success check is shown and their boxes and target classes (ViewRows), and the verdict
behind a stage's detections (verdict_of).  detector_loss, set_detector, roi_detector, proposals and detector_output
take them from here; a new adapter does too.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from diff_gaussian_rasterization import detect_ops


def gt_rows(gt_boxes, gt_cls, device, affine: Tuple[float, float, float] = (1.0, 0.0, 0.0)) -> Tuple[torch.Tensor, torch.Tensor]:
    """gt_boxes [B,M,4] / gt_cls [B,M], or [B,4] / [B]: one row per image -> (float32 [B,M,4], int32 [B,M]) on `device`.
    gt_cls None: every row present (class 0).  affine (scale, shift_x, shift_y): boxes' = boxes * scale + shift.  A row
    holding a NaN is absent: class -1, box zeroed."""
    gb = torch.as_tensor(gt_boxes, dtype=torch.float32).to(device)
    if gb.dim() == 2:
        gb = gb[:, None, :]
    if gt_cls is None:
        gc = torch.zeros(gb.shape[:2], dtype=torch.int32, device=device)
    else:
        gc = torch.as_tensor(gt_cls).to(device=device, dtype=torch.int32)
        if gc.numel() == gb.shape[0] * gb.shape[1]:
            gc = gc.reshape(gb.shape[:2])
    s, ox, oy = affine
    if (s, ox, oy) != (1.0, 0.0, 0.0):
        gb = gb * s + torch.tensor([ox, oy, ox, oy], dtype=torch.float32, device=device)
    gc = torch.where(torch.isnan(gb).any(-1), torch.full_like(gc, -1), gc)
    return torch.nan_to_num(gb, nan=0.0), gc


class ViewRows:
    """gt_bboxes [V,4] (or None): every view's box; target: the class of every view, one int or one per view (or None).
    Called with what pgd_attack hands a loss_fn -- renders [B,3,H,W] (or [3,H,W]) and idx, the global view indices of
    the renders (default 0..B-1) -- it returns (renders [B,3,H,W], gt [B,4] or None, classes int32 [B] or None)."""

    def __init__(self, gt_bboxes, target=None):
        self.gt = None if gt_bboxes is None else torch.as_tensor(gt_bboxes, dtype=torch.float32)
        self.target = None if target is None else torch.as_tensor(target, dtype=torch.int32)

    def __call__(self, renders: torch.Tensor, idx: Optional[Sequence[int]] = None):
        x = renders[None] if renders.dim() == 3 else renders
        ids = list(range(int(x.shape[0]))) if idx is None else [int(i) for i in idx]
        if len(ids) != int(x.shape[0]):
            raise ValueError(f"loss_fn: {len(ids)} view indices for {int(x.shape[0])} renders")
        gt = None if self.gt is None else self.gt[ids]
        if self.target is None:
            return x, gt, None
        return x, gt, self.target.expand(len(self.gt))[ids] if self.target.dim() == 0 else self.target[ids]


def verdict_of(dets: torch.Tensor, counts: torch.Tensor, gt_bboxes, target: int, untarget: Optional[int] = None,
               is_targeted: bool = True, iou_match: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tail of every stage's verdict: gt_bboxes [B,4] (None or a NaN row: no box for that view) to the detections'
    device, then gsr_det_verdict -> (flags int32 [B]: bit 0 success, bit 1 target_exists, bit 2 untarget_absent; best [B,4])."""
    gt = None if gt_bboxes is None else torch.as_tensor(gt_bboxes, dtype=torch.float32).to(dets.device)
    return detect_ops.verdict(dets, counts, gt, target, untarget, is_targeted, iou_match)

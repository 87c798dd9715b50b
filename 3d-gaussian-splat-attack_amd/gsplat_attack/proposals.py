"""The region proposer of a two-stage (R-CNN-style) detector, on the RPN proposal stage's HIP kernels
(diff_gaussian_rasterization.rpn_ops): the step between the RPN head and gsplat_attack.roi_detector's sampler.

The reference's default detector (Detectron2's Faster R-CNN in its C4 form, run in training mode by infer()) takes, per
image and PGD step, the best 12 000 of 15 * Hf * Wf objectness logits, decodes them against their anchors, clips, runs NMS
at 0.7 and keeps 2 000.  torch.topk and torchvision's NMS leave the order of ties open; here ties are decided by index and
by slot, so the proposals -- and with them the RoIs the sampler draws -- are the same bits on every run.
include/gsraster.h holds the formulas; INTEGRATION.md section 8i lists the stated deviations.

  cell_anchors   (sizes, aspect_ratios) -> [A,4]: Detectron2's generate_cell_anchors
  RpnProposer    .propose(logits, deltas) -> Proposals(boxes, scores, counts); with a `head`, a callable for
                 make_roi_loss_fn: proposer(features) -> (boxes [B,R,4], counts [B])
  RpnLoss        .loss(logits, deltas, gt_boxes, gt_cls=None) -> (total, terms[2] = cls, loc): the two RPN losses on
                 diff_gaussian_rasterization.rpnloss_ops; .labels(sizes, gt_boxes, gt_cls=None) -> the anchors' labels alone;
                 make_roi_loss_fn(..., rpn_loss=...) adds its total to the box head's loss
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from diff_gaussian_rasterization import rpn_ops, rpnloss_ops
from diff_gaussian_rasterization.rpn_ops import RpnSpec
from diff_gaussian_rasterization.rpnloss_ops import RpnLossSpec

from ._views import gt_rows


class Proposals(NamedTuple):
    """boxes [B,R,4] x1 y1 x2 y2 in image pixels, best first, zero rows beyond the count; scores [B,R]: their objectness
    logits; counts int32 [B]."""
    boxes: torch.Tensor
    scores: torch.Tensor
    counts: torch.Tensor


def cell_anchors(sizes: Sequence[float], aspect_ratios: Sequence[float]) -> torch.Tensor:
    """Detectron2's DefaultAnchorGenerator.generate_cell_anchors: for every size, for every aspect ratio (h / w), the box of
    area size^2 centred on 0 -- computed in Python doubles and cast to float32, as Detectron2 does.  -> [A,4] on the CPU."""
    rows = []
    for size in sizes:
        area = float(size) ** 2.0
        for ratio in aspect_ratios:
            w = math.sqrt(area / float(ratio))
            h = float(ratio) * w
            rows.append([-w / 2.0, -h / 2.0, w / 2.0, h / 2.0])
    if not rows:
        raise ValueError("cell_anchors: at least one size and one aspect ratio")
    return torch.tensor(rows, dtype=torch.float32)


LevelDef = Tuple[torch.Tensor, int, float]


class RpnProposer:
    """levels: one (cell_anchors [A,4], stride, offset) per feature level, in the head's order (offset: Detectron2's anchor
    offset, 0 by default there); frame = (img_w, img_h): the boxes are clipped to it; pre_topk per level and post_topk in
    all (Detectron2 in training: 12 000, 2 000; at most 4096 come out, what the sampler can take); nms: the IoU threshold;
    min_size: both sides of a box must exceed it.  head: optional, features -> (logits, deltas), tensors or per-level
    lists; with it the proposer is a callable for make_roi_loss_fn."""

    def __init__(self, levels: Sequence[LevelDef], frame: Tuple[float, float], pre_topk: int = 12000, post_topk: int = 2000,
                 nms: float = 0.7, min_size: float = 0.0, head: Optional[Callable] = None):
        w, h = float(frame[0]), float(frame[1])
        if not (w > 0 and h > 0 and math.isfinite(w) and math.isfinite(h)):
            raise ValueError("RpnProposer: frame must be (img_w, img_h) with both finite and > 0")
        if len(levels) < 1:
            raise ValueError("RpnProposer: at least one level")
        if not 1 <= int(pre_topk) <= rpn_ops.MAX_SLOTS:
            raise ValueError(f"RpnProposer: pre_topk must be 1..{rpn_ops.MAX_SLOTS}")
        if not 1 <= int(post_topk) <= rpn_ops.MAX_POST:
            raise ValueError(f"RpnProposer: post_topk must be 1..{rpn_ops.MAX_POST}")
        if not (0.0 <= float(nms) < float("inf")) or not (0.0 <= float(min_size) < float("inf")):
            raise ValueError("RpnProposer: nms and min_size must be finite and >= 0")
        self.levels = []
        for lv in levels:
            ca, stride = torch.as_tensor(lv[0], dtype=torch.float32), int(lv[1])
            offset = float(lv[2]) if len(lv) > 2 else 0.0
            if ca.dim() != 2 or ca.shape[1] != 4 or ca.shape[0] < 1 or stride < 1:
                raise ValueError("RpnProposer: a level is (cell_anchors [A,4], stride >= 1, offset)")
            self.levels.append((ca, stride, offset))
        self.spec = RpnSpec(img_w=w, img_h=h, min_size=float(min_size), pre_topk=int(pre_topk), post_topk=int(post_topk),
                            iou_thr=float(nms))
        self.head = head

    def _per_level(self, x: Union[torch.Tensor, Sequence[torch.Tensor]], name: str):
        xs = [x] if isinstance(x, torch.Tensor) else list(x)
        if len(xs) != len(self.levels):
            raise ValueError(f"RpnProposer: {len(xs)} {name} tensors for {len(self.levels)} levels")
        return xs

    def propose(self, logits, deltas) -> Proposals:
        """logits [B,A,Hf,Wf] and deltas [B,4A,Hf,Wf], or one of each per level -> Proposals."""
        lg, dl = self._per_level(logits, "logits"), self._per_level(deltas, "deltas")
        lvs = []
        for i, (l, d) in enumerate(zip(lg, dl)):
            ca, stride, offset = self.levels[i]
            if ca.device != l.device:                                      # moved once, kept
                ca = ca.to(l.device)
                self.levels[i] = (ca, stride, offset)
            lvs.append(rpn_ops.Level(l, d, ca, stride, offset))
        out = rpn_ops.propose(lvs, self.spec)
        return Proposals(out.boxes, out.scores, out.counts)

    def __call__(self, features) -> Tuple[torch.Tensor, torch.Tensor]:
        """For make_roi_loss_fn: features -> (boxes [B,R,4], counts [B]) through the head given at construction."""
        if self.head is None:
            raise RuntimeError("RpnProposer: calling the proposer on features needs the RPN head it was built with (head=...)")
        logits, deltas = self.head(features)
        p = self.propose(logits, deltas)
        return p.boxes, p.counts


class RpnLoss:
    """The two RPN losses (Detectron2's loss_rpn_cls and loss_rpn_loc) on the RPN loss stage's HIP kernels
    (diff_gaussian_rasterization.rpnloss_ops): the only losses that act on the proposal stage itself.  levels: one
    (cell_anchors [A,4], stride, offset) per feature level, in the head's order, as RpnProposer takes them;
    batch_per_image anchors are sampled per image, at most int(batch_per_image * positive_fraction) of them positive
    (Detectron2: 256, 0.5); iou = (lo, hi): an anchor whose best IoU is below lo is negative, from hi on positive, between
    them ignored (0.3, 0.7); cls, loc: the weights of the two terms; beta: smooth L1's (0: plain L1); seed: the key of the
    sample, which takes the place of Detectron2's randperm -- the same seed draws the same anchors on every run.
    include/gsraster.h holds the formulas; INTEGRATION.md section 8l lists the stated deviations."""

    def __init__(self, levels: Sequence[LevelDef], batch_per_image: int = 256, positive_fraction: float = 0.5,
                 iou: Tuple[float, float] = (0.3, 0.7), cls: float = 1.0, loc: float = 1.0, beta: float = 0.0, seed: int = 0):
        if len(levels) < 1 or len(levels) > rpnloss_ops.MAX_LEVELS:
            raise ValueError(f"RpnLoss: 1..{rpnloss_ops.MAX_LEVELS} levels")
        if not 1 <= int(batch_per_image) <= rpnloss_ops.MAX_BATCH:
            raise ValueError(f"RpnLoss: batch_per_image must be 1..{rpnloss_ops.MAX_BATCH}")
        if not 0.0 <= float(positive_fraction) <= 1.0:
            raise ValueError("RpnLoss: positive_fraction must be in [0, 1]")
        lo, hi = float(iou[0]), float(iou[1])
        if not (0.0 <= lo <= hi < float("inf")):
            raise ValueError("RpnLoss: iou must be (lo, hi) with 0 <= lo <= hi, both finite")
        if not all(0.0 <= float(v) < float("inf") for v in (cls, loc, beta)):
            raise ValueError("RpnLoss: the weights and beta must be finite and >= 0")
        self.levels = []
        for lv in levels:
            ca, stride = torch.as_tensor(lv[0], dtype=torch.float32), int(lv[1])
            offset = float(lv[2]) if len(lv) > 2 else 0.0
            if ca.dim() != 2 or ca.shape[1] != 4 or ca.shape[0] < 1 or stride < 1:
                raise ValueError("RpnLoss: a level is (cell_anchors [A,4], stride >= 1, offset)")
            self.levels.append((ca, stride, offset))
        self.spec = RpnLossSpec(batch_per_image=int(batch_per_image), pos_quota=int(int(batch_per_image) * float(positive_fraction)),
                                seed=int(seed), iou_lo=lo, iou_hi=hi, beta=float(beta), w_cls=float(cls), w_loc=float(loc))

    def _per_level(self, x, name: str):
        xs = [x] if isinstance(x, torch.Tensor) else list(x)
        if len(xs) != len(self.levels):
            raise ValueError(f"RpnLoss: {len(xs)} {name} for {len(self.levels)} levels")
        return xs

    def _anchor_levels(self, sizes, device):
        out = []
        for i, hw in enumerate(sizes):
            ca, stride, offset = self.levels[i]
            if ca.device != device:                                        # moved once, kept
                ca = ca.to(device)
                self.levels[i] = (ca, stride, offset)
            out.append(rpnloss_ops.AnchorLevel(ca, stride, (int(hw[0]), int(hw[1])), offset))
        return out

    def labels(self, sizes, gt_boxes, gt_cls=None, seed: Optional[int] = None, want_pre: bool = False) -> "rpnloss_ops.Labels":
        """sizes: one (Hf, Wf) per level (or the logits themselves); gt_boxes on the device the labels are wanted on ->
        rpnloss_ops.Labels(labels, matched, counts, prelabels)."""
        device = torch.as_tensor(gt_boxes).device
        hw = [tuple(s.shape[-2:]) if isinstance(s, torch.Tensor) else tuple(s) for s in self._per_level(sizes, "sizes")]
        gb, gc = gt_rows(gt_boxes, gt_cls, device)
        spec = self.spec if seed is None else self.spec._replace(seed=int(seed))
        return rpnloss_ops.label(self._anchor_levels(hw, device), gb, gc, spec, want_pre=want_pre)

    def loss(self, logits, deltas, gt_boxes, gt_cls=None, seed: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """logits [B,A,Hf,Wf] and deltas [B,4A,Hf,Wf], or one of each per level -> (total, terms[2] = cls, loc as they enter
        the total); total is differentiable with respect to the logits and the deltas."""
        lg, dl = self._per_level(logits, "logits"), self._per_level(deltas, "deltas")
        device = lg[0].device
        gb, gc = gt_rows(gt_boxes, gt_cls, device)
        spec = self.spec if seed is None else self.spec._replace(seed=int(seed))
        return rpnloss_ops.rpn_loss(lg, dl, self._anchor_levels([tuple(x.shape[-2:]) for x in lg], device), gb, gc, spec)

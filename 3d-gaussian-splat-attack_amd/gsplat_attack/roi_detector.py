"""Both sides of a two-stage (R-CNN-style) detector, on the two-stage stage's HIP kernels
(diff_gaussian_rasterization.rcnn_ops).  Such a detector runs a backbone to one feature map, takes proposals from a region
proposer, pools every proposal with RoIAlign and hands the pooled features to a box head that emits C + 1 class scores
(the last: background) and 4 box deltas per class for every RoI.

The reference's default detector is Detectron2's Faster R-CNN in its C4 form (detectors/detectron2_detector.py): its
infer() descends on loss_cls of 512 RoIs per image drawn by a host randperm, through a RoIAlign whose backward scatters
with float atomics.  Here the sample is a keyed, fixed draw, RoIAlign's backward is a gather and the loss a fixed-order
sum, so that a PGD step is bitwise reproducible from the loss back to the Gaussian parameters.  include/gsraster.h holds
the formulas; INTEGRATION.md lists the stated deviations.

  ProposalSampler   .sample(proposals, gt_boxes, gt_cls, seed=...) -> rcnn_ops.Sample
  roi_align         (features, rois, counts, ...) -> pooled [B,S,Cf,PH,PW], differentiable with respect to the features
  FpnRoIPooler      (features of a pyramid, rois, counts) -> pooled: every RoI from the level its size picks (Detectron2's
                    ROIPooler), on diff_gaussian_rasterization.fpn_ops; .levels(rois, counts) -> the levels alone
  RoIHeadLoss       .loss(scores, deltas, sample, gt_boxes) -> (total, items[2] = cls, box)
  RoIHeadOutput     .detect(scores, deltas, proposals) -> (dets, counts); .verdicts(...) on gsr_det_verdict
  make_roi_loss_fn  renders -> detector_input -> backbone -> proposer (detached; gsplat_attack.proposals.RpnProposer is one)
                    -> sample -> roi_align (or, with pooler=..., an FpnRoIPooler on a pyramid) -> box_head -> loss
                    as pgd_attack's loss_fn; it takes the global view indices of the renders (loss_fn.takes_view_index);
                    with rpn_loss=... (a gsplat_attack.proposals.RpnLoss) the RPN head runs with gradient and the two RPN
                    losses are added
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple, Union

import torch

from diff_gaussian_rasterization import fpn_ops, rcnn_ops
from diff_gaussian_rasterization.rcnn_ops import RcnnSpec, Sample

from ._views import ViewRows, gt_rows, verdict_of


class ProposalSampler:
    """nc classes; per_image RoIs per image of which at most positive_fraction are foreground (Detectron2: 512, 0.25);
    fg_iou: the IoU from which a candidate is foreground; append_gt: the ground-truth boxes are candidates too."""

    def __init__(self, nc: int, per_image: int = 512, positive_fraction: float = 0.25, fg_iou: float = 0.5, append_gt: bool = True,
                 seed: int = 0):
        if not 1 <= nc <= rcnn_ops.MAX_CLASSES:
            raise ValueError(f"ProposalSampler: nc must be 1..{rcnn_ops.MAX_CLASSES}")
        if not 1 <= per_image <= rcnn_ops.MAX_SAMPLE:
            raise ValueError(f"ProposalSampler: per_image must be 1..{rcnn_ops.MAX_SAMPLE}")
        if not 0.0 <= positive_fraction <= 1.0:
            raise ValueError("ProposalSampler: positive_fraction must be in [0, 1]")
        self.nc = int(nc)
        self.seed = int(seed)
        self.spec = RcnnSpec(S=int(per_image), max_pos=int(per_image * positive_fraction), append_gt=bool(append_gt),
                             fg_iou=float(fg_iou))

    def sample(self, proposals: torch.Tensor, gt_boxes, gt_cls, seed: Optional[int] = None,
               n_prop: Optional[torch.Tensor] = None) -> Sample:
        """proposals [B,R,4] x1 y1 x2 y2 in pixels, in the proposer's order; gt_boxes [B,M,4] (or [B,4]); gt_cls [B,M] (or [B]),
        negative: absent.  The same seed gives the same sample; pass a new one for a fresh draw."""
        gb, gc = gt_rows(gt_boxes, gt_cls, proposals.device)
        spec = self.spec._replace(seed=self.seed if seed is None else int(seed))
        return rcnn_ops.sample(proposals, gb, gc, self.nc, spec, n_prop=n_prop)


def roi_align(features: torch.Tensor, rois: torch.Tensor, counts: Optional[torch.Tensor] = None, output_size=(14, 14),
              spatial_scale: float = 1.0 / 16.0, sampling_ratio: int = 0) -> torch.Tensor:
    """Detectron2's ROIAlignV2 (aligned): features [B,Cf,Hf,Wf], rois [B,S,4] in image pixels, counts: a Sample's counts
    (or int32 [B], or None: every row) -> pooled [B,S,Cf,PH,PW]; rows beyond the count are zero."""
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    spec = RcnnSpec(PH=int(ph), PW=int(pw), spatial_scale=float(spatial_scale), sampling_ratio=int(sampling_ratio))
    return rcnn_ops.roi_align(features, rois, counts, spec)


class FpnRoIPooler:
    """Detectron2's ROIPooler (ROIAlignV2) on a feature pyramid: strides, finest first, powers of two and each double the
    last (p2..p5: 4, 8, 16, 32); a RoI of size sqrt(area) = canonical_size belongs to the level of stride
    2^canonical_level, one of half that size to the level below, and so on, clamped to the levels there are.  The level
    comes from thresholds on sqrt(area) / canonical_size, not from a logarithm: INTEGRATION.md section 8j."""

    def __init__(self, strides: Sequence[int] = (4, 8, 16, 32), output_size=7, sampling_ratio: int = 0, canonical_size: float = 224.0,
                 canonical_level: int = 4):
        st = [int(v) for v in strides]
        if not 1 <= len(st) <= fpn_ops.MAX_LEVELS:
            raise ValueError(f"FpnRoIPooler: 1..{fpn_ops.MAX_LEVELS} strides")
        if any(v < 1 or v & (v - 1) for v in st) or any(b != 2 * a for a, b in zip(st, st[1:])):
            raise ValueError("FpnRoIPooler: the strides must be powers of two, each double the last")
        ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
        if not (1 <= int(ph) <= fpn_ops.MAX_POOL and 1 <= int(pw) <= fpn_ops.MAX_POOL) or int(sampling_ratio) < 0:
            raise ValueError(f"FpnRoIPooler: output_size must be 1..{fpn_ops.MAX_POOL} each and sampling_ratio >= 0")
        if not (0.0 < float(canonical_size) < float("inf")):
            raise ValueError("FpnRoIPooler: canonical_size must be finite and > 0")
        self.strides = tuple(st)
        self.spec = fpn_ops.FpnSpec(scales=tuple(1.0 / v for v in st), thr=fpn_ops.level_thresholds(st, int(canonical_level)),
                                    PH=int(ph), PW=int(pw), sampling_ratio=int(sampling_ratio), canonical_size=float(canonical_size))

    def _maps(self, features) -> list:
        maps = [features] if isinstance(features, torch.Tensor) else list(features)
        if len(maps) != len(self.strides):
            raise ValueError(f"FpnRoIPooler: {len(maps)} feature maps for {len(self.strides)} strides")
        return maps

    def __call__(self, features, rois: torch.Tensor, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """features: one [B,Cf,Hf_l,Wf_l] per stride; rois [B,S,4] in image pixels; counts: a Sample's counts (or int32 [B], or
        None: every row) -> pooled [B,S,Cf,PH,PW], differentiable with respect to every map; rows without a level are zero."""
        return fpn_ops.fpn_pool(self._maps(features), rois, counts, self.spec)

    def levels(self, rois: torch.Tensor, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> int32 [B,S]: the index into strides of every RoI's level; -1 beyond the count and for a non-finite row."""
        B = int(rois.shape[0])
        maps = [torch.zeros((B, 1, 1, 1), dtype=torch.float32, device=rois.device) for _ in self.strides]
        return fpn_ops.pool_forward(maps, rois, counts, self.spec._replace(PH=1, PW=1, sampling_ratio=1))[1]


class RoIHeadLoss:
    """nc classes (the head emits nc + 1 scores per RoI); cls, box: the weights of the two terms -- the reference descends on
    the classification term alone (1, 0); Detectron2's own sum is (1, 1)."""

    def __init__(self, nc: int, cls: float = 1.0, box: float = 0.0, box_weights=(10.0, 10.0, 5.0, 5.0), beta: float = 0.0,
                 class_agnostic: bool = False):
        if not 1 <= nc <= rcnn_ops.MAX_CLASSES:
            raise ValueError(f"RoIHeadLoss: nc must be 1..{rcnn_ops.MAX_CLASSES}")
        vals = (cls, box, beta)
        if not all(float(v) >= 0 and float(v) < float("inf") for v in vals):
            raise ValueError("RoIHeadLoss: the weights and beta must be finite and >= 0")
        self.nc = int(nc)
        self.spec = RcnnSpec(w_cls=float(cls), w_box=float(box), box_weights=tuple(float(v) for v in box_weights), beta=float(beta),
                             class_agnostic=bool(class_agnostic))

    def loss(self, scores: torch.Tensor, deltas: torch.Tensor, sample: Sample, gt_boxes) -> Tuple[torch.Tensor, torch.Tensor]:
        """scores [B,S,nc+1]; deltas [B,S,4*nc] (or [B,S,4]); sample: what ProposalSampler.sample returned; gt_boxes as given
        to it -> (total, items[2] = cls, box unweighted)."""
        if scores.dim() != 3 or scores.shape[2] != self.nc + 1:
            raise ValueError(f"RoIHeadLoss: scores must be [B,S,{self.nc + 1}], got {tuple(scores.shape)}")
        gb = torch.as_tensor(gt_boxes, dtype=torch.float32).to(scores.device)
        if gb.dim() == 2:
            gb = gb[:, None, :]
        gb = torch.nan_to_num(gb, nan=0.0)
        return rcnn_ops.rcnn_loss(scores, deltas, sample.rois, sample.labels, sample.gt_row, gb, self.spec)


class RoIHeadOutput:
    """frame = (img_w, img_h): the boxes are clipped to it; conf: the score a proposal must exceed (the reference: 0.5);
    iou: the NMS threshold; max_det: rows per image (Detectron2: 100)."""

    def __init__(self, frame: Tuple[float, float], conf: float = 0.5, iou: float = 0.5, max_det: int = 100,
                 box_weights=(10.0, 10.0, 5.0, 5.0), class_agnostic: bool = False):
        w, h = float(frame[0]), float(frame[1])
        if not (w > 0 and h > 0):
            raise ValueError("frame must be (img_w, img_h) with both > 0")
        if not 1 <= max_det <= rcnn_ops.MAX_CAND:
            raise ValueError(f"RoIHeadOutput: max_det must be 1..{rcnn_ops.MAX_CAND}")
        self.spec = RcnnSpec(conf_thr=float(conf), iou_thr=float(iou), max_det=int(max_det), img_w=w, img_h=h,
                             box_weights=tuple(float(v) for v in box_weights), class_agnostic=bool(class_agnostic))

    def detect(self, scores: torch.Tensor, deltas: torch.Tensor, proposals: torch.Tensor,
               n_prop: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (dets [B,min(max_det,R),6]: x1 y1 x2 y2 score class of the kept boxes, best first, zero rows beyond; counts int32
        [B,2]: kept, candidates), both on the scores' device."""
        return rcnn_ops.postprocess(scores, deltas, proposals, self.spec, n_prop=n_prop)

    def verdicts(self, scores: torch.Tensor, deltas: torch.Tensor, proposals: torch.Tensor, gt_bboxes: Optional[torch.Tensor],
                 target: int, untarget: Optional[int] = None, is_targeted: bool = True, iou_match: float = 0.5,
                 n_prop: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """gt_bboxes [B,4] (x1 y1 x2 y2 in the frame; None or a NaN row: no box for that view)
        -> (flags int32 [B] on the device: bit 0 success, bit 1 target_exists, bit 2 untarget_absent;
            best [B,4]: iou, score, class, row of the detection closest to the gt box, -1 where there is none)."""
        dets, counts = self.detect(scores, deltas, proposals, n_prop=n_prop)
        return verdict_of(dets, counts, gt_bboxes, target, untarget, is_targeted, iou_match)


def make_roi_loss_fn(backbone: Callable, proposer: Callable, box_head: Callable, detector_input: Optional[Callable],
                     sampler: ProposalSampler, head_loss: RoIHeadLoss, gt_bboxes, target: Union[int, Sequence[int]],
                     output_size=(14, 14), spatial_scale: float = 1.0 / 16.0, sampling_ratio: int = 0,
                     pooler: Optional[Callable] = None, rpn_loss=None) -> Callable:
    """-> loss_fn(renders [B,3,H,W], idx=None) -> total, for pgd_attack(loss_fn=...).  backbone(images) -> features
    [B,Cf,Hf,Wf]; proposer(features) -> proposals [B,R,4] in image pixels (taken detached, as Detectron2 does), or
    (proposals, n_prop int32 [B]) where only the first n_prop[b] rows of image b are proposals, as a
    gsplat_attack.proposals.RpnProposer returns them;
    box_head(pooled [B*S,Cf,PH,PW]) -> (scores [B*S,nc+1], deltas [B*S,4*nc or 4]); gt_bboxes [V,4]: every view's box in the
    frame of the detector's input; target: the class the loss pulls towards, one int or one per view; idx: the views the
    renders show (default 0..B-1).  The sampler's seed is its own: every step draws the same RoIs for the same proposals.
    pooler: an FpnRoIPooler (or any (features, rois, counts) -> pooled); then backbone may return a sequence of maps, the
    proposer receives each of them detached, and output_size, spatial_scale and sampling_ratio are the pooler's own.
    rpn_loss: a gsplat_attack.proposals.RpnLoss; then the proposer must be an RpnProposer built with its head: the head runs
    once WITH gradient, its detached outputs go to proposer.propose, and rpn_loss's total (every view's box as its one gt
    row, a NaN row absent) is added to the box head's loss -- the only path from the RPN head back to the renders."""
    if rpn_loss is not None and getattr(proposer, "head", None) is None:
        raise ValueError("make_roi_loss_fn: rpn_loss needs a proposer with .head and .propose (an RpnProposer built with head=...)")
    views = ViewRows(gt_bboxes, target)

    def loss_fn(renders: torch.Tensor, idx: Optional[Sequence[int]] = None) -> torch.Tensor:
        x, gt, cls = views(renders, idx)
        features = backbone(detector_input(x) if detector_input is not None else x)
        rpn_logits = rpn_deltas = None
        if rpn_loss is not None:                                         # the head once, with gradient; the proposals from its detached outputs
            rpn_logits, rpn_deltas = proposer.head(features)
            with torch.no_grad():
                det = lambda v: v.detach() if isinstance(v, torch.Tensor) else [t.detach() for t in v]
                p = proposer.propose(det(rpn_logits), det(rpn_deltas))
                proposals = (p.boxes, p.counts)
        else:
            with torch.no_grad():
                if pooler is not None and not isinstance(features, torch.Tensor):
                    proposals = proposer([f.detach() for f in features])
                else:
                    proposals = proposer(features.detach())
        n_prop = None
        if not isinstance(proposals, torch.Tensor):                      # (proposals, n_prop): rows beyond the count are no candidates
            proposals, n_prop = proposals
        smp = sampler.sample(proposals, gt, cls, n_prop=n_prop)
        if pooler is not None:
            pooled = pooler(features, smp.rois, smp.counts)
        else:
            pooled = roi_align(features, smp.rois, smp.counts, output_size, spatial_scale, sampling_ratio)
        B, S = int(pooled.shape[0]), int(pooled.shape[1])
        scores, deltas = box_head(pooled.reshape(B * S, *pooled.shape[2:]))
        total = head_loss.loss(scores.reshape(B, S, -1), deltas.reshape(B, S, -1), smp, gt)[0]
        if rpn_loss is None:
            return total
        return total + rpn_loss.loss(rpn_logits, rpn_deltas, gt.to(total.device))[0]

    loss_fn.takes_view_index = True
    return loss_fn

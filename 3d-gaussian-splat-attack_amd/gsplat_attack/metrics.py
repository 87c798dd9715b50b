"""Scoring an attack: the counterpart of the reference's evaluation sweep (utils/render.py:223-298) and of the two scripts that
read its log, utils/analyze_ap_ar.py (pycocotools' COCOeval: AP@0.5 over all areas with 100 detections, AR@0.5 with one) and
utils/analyze_asr.py (the attack success rate).

  DetectionEval        COCOeval for boxes on the device: update() per batch of dets / counts as any detector output stage writes
                       them, compute() -> precision, recall, scores, npig and the 14 statistics; the same bits on every run
  reference_eval       the reference's set-up (params.iouThrs = [iou_thr])
  attack_success_rate  from gsr_det_verdict's words of a benign and an adversarial sweep
  evaluate_views       the sweep: render, detect, verdict, metrics, one record per camera
  to_coco_json / from_coco_json   the two files of build_coco_jsons, for a machine that has pycocotools, and back

Deviations from COCOeval: a NaN IoU counts as 0, no crowd / ignore annotations, dead rows (a NaN,
a class outside 0..K-1, beyond the count) take no part, ties are broken by row / image order, caps and areas go by position.
"""
from __future__ import annotations

import json
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from diff_gaussian_rasterization import deteval_ops
from diff_gaussian_rasterization.deteval_ops import STAT_NAMES, EvalSpec, MatchOut

from ._views import gt_rows, verdict_of

COCO_AREA_RANGES = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))
TARGET_EXISTS = 2            # bit 1 of gsr_det_verdict's word


class DetectionEval:
    """COCOeval(iouType='bbox') without crowd annotations.  The thresholds are float64 arrays the kernels compare against as
    they are (numpy.linspace(0, 1, 101)[i] and i / 100.0 differ in the last bit for some i)."""

    def __init__(self, num_classes: int, iou_thrs=None, rec_thrs=None, area_ranges=COCO_AREA_RANGES, max_dets: Sequence[int] = (1, 10, 100)):
        self.num_classes = int(num_classes)
        self.iou_thrs = np.asarray(np.linspace(0.5, 0.95, 10) if iou_thrs is None else iou_thrs, dtype=np.float64).reshape(-1)
        self.rec_thrs = np.asarray(np.linspace(0.0, 1.0, 101) if rec_thrs is None else rec_thrs, dtype=np.float64).reshape(-1)
        self.area_ranges = tuple((float(lo), float(hi)) for lo, hi in area_ranges)
        self.max_dets = tuple(int(c) for c in max_dets)
        if not 1 <= self.num_classes <= deteval_ops.MAX_K:
            raise ValueError(f"DetectionEval: num_classes={num_classes} (1..{deteval_ops.MAX_K})")
        if not 1 <= len(self.iou_thrs) <= deteval_ops.MAX_T or not 1 <= len(self.rec_thrs) <= deteval_ops.MAX_R \
                or not 1 <= len(self.area_ranges) <= deteval_ops.MAX_A or not 1 <= len(self.max_dets) <= deteval_ops.MAX_CAPS:
            raise ValueError(f"DetectionEval: {len(self.iou_thrs)} IoU thresholds (1..{deteval_ops.MAX_T}), {len(self.rec_thrs)} recall "
                             f"thresholds (1..{deteval_ops.MAX_R}), {len(self.area_ranges)} area ranges (1..{deteval_ops.MAX_A}), "
                             f"{len(self.max_dets)} max_dets (1..{deteval_ops.MAX_CAPS})")
        if any(c < 1 for c in self.max_dets) or list(self.max_dets) != sorted(self.max_dets):
            raise ValueError(f"DetectionEval: max_dets={self.max_dets} must be positive and ascending")
        self.reset()

    def reset(self) -> None:
        self._dets: List[torch.Tensor] = []
        self._gt_cls: List[torch.Tensor] = []
        self._match: List[MatchOut] = []

    def spec(self, D: int) -> EvalSpec:
        """A cap above D admits every detection of an image, as the cap D does."""
        return EvalSpec(self.num_classes, tuple(self.iou_thrs.tolist()), self.area_ranges, tuple(min(c, int(D)) for c in self.max_dets),
                        len(self.rec_thrs))

    @property
    def num_images(self) -> int:
        return sum(int(d.shape[0]) for d in self._dets)

    def update(self, dets: torch.Tensor, counts: torch.Tensor, gt_boxes, gt_cls=None) -> MatchOut:
        """dets [B,D,6] / counts [B,2] of a detector output stage; gt_boxes [B,M,4] with gt_cls [B,M], or [B,4] with [B] (or None:
        class 0): x1 y1 x2 y2 in the frame of dets.  A ground-truth row holding a NaN, or of a class outside 0..K-1, is absent.
        Runs the match and keeps its outputs on the device."""
        deteval_ops._check_dets("DetectionEval.update", dets)
        if self._dets and (self._dets[0].shape[1] != dets.shape[1] or self._dets[0].device != dets.device):
            raise ValueError(f"DetectionEval.update: dets {tuple(dets.shape)} on {dets.device} after {tuple(self._dets[0].shape)} on "
                             f"{self._dets[0].device}: one evaluation has one D and one device")
        gb, gc = gt_rows(gt_boxes, gt_cls, dets.device)
        d = dets.detach().to(torch.float32).contiguous()
        m = deteval_ops.match(d, counts, gb, gc, self.spec(int(d.shape[1])))
        self._dets.append(d)
        self._gt_cls.append(gc)
        self._match.append(m)
        return m

    def compute(self) -> Dict[str, object]:
        """Accumulates over everything seen -> precision, scores [T,R,K,A,Mx], recall [T,K,A,Mx], npig [K,A] (device tensors) and
        stats: COCO's twelve names plus ap_ref and ar_ref (floats; the call's one read-back)."""
        if not self._dets:
            raise RuntimeError("DetectionEval.compute: no update() yet")
        dev = self._dets[0].device
        M = max(int(g.shape[1]) for g in self._gt_cls)

        def pad(t: torch.Tensor, value: int) -> torch.Tensor:          # batches of fewer ground-truth rows: absent rows behind them
            return t if t.shape[-1] == M else torch.nn.functional.pad(t, (0, M - t.shape[-1]), value=value)
        dets = torch.cat(self._dets)
        gt_cls = torch.cat([pad(g, -1) for g in self._gt_cls])
        m = MatchOut(*(torch.cat([pad(getattr(b, f), v) if f.startswith("gt_") else getattr(b, f) for b in self._match])
                       for f, v in zip(MatchOut._fields, (0, 0, 0, 0, 2, -1))))
        spec = self.spec(int(dets.shape[1]))
        rec = torch.from_numpy(self.rec_thrs.copy()).to(dev)
        precision, scores, recall, npig = deteval_ops.accumulate(dets, m, gt_cls, rec, spec)
        stats = deteval_ops.summarize(precision, recall, spec)
        return dict(precision=precision, scores=scores, recall=recall, npig=npig, stats_tensor=stats,
                    stats=dict(zip(STAT_NAMES, stats.cpu().tolist())))


def reference_eval(iou_thr: float = 0.5, num_classes: int = 80) -> DetectionEval:
    """utils/analyze_ap_ar.py:150-161: COCOeval with params.iouThrs = [iou_thr]; its two numbers are stats['ap_ref'] and
    stats['ar_ref']."""
    return DetectionEval(num_classes, iou_thrs=[float(iou_thr)])


def attack_success_rate(benign_verdict, adv_verdict) -> Tuple[int, int, float]:
    """utils/analyze_asr.py:46-53 from gsr_det_verdict's words: total = the views whose benign prediction is the target class (bit 1,
    target_exists), successful = those of them whose adversarial prediction is not -> (successful, total, rate); rate 0.0 when total
    is 0."""
    b = torch.as_tensor(benign_verdict).to(torch.int64).reshape(-1).cpu()
    a = torch.as_tensor(adv_verdict).to(torch.int64).reshape(-1).cpu()
    if b.shape != a.shape:
        raise ValueError(f"attack_success_rate: {b.numel()} benign and {a.numel()} adversarial verdicts")
    hit = (b & TARGET_EXISTS) != 0
    total = int(hit.sum())
    successful = int((hit & ((a & TARGET_EXISTS) == 0)).sum())
    return successful, total, (successful / total if total else 0.0)


def _xywh(box) -> List[float]:
    """x1 y1 x2 y2 -> [x, y, w, h] rounded to 0.1 (detectors/yolov5_detector.py:180, 217)"""
    x1, y1, x2, y2 = (float(v) for v in box)
    return [round(x1, 1), round(y1, 1), round(x2 - x1, 1), round(y2 - y1, 1)]


def view_records(dets: torch.Tensor, best: torch.Tensor, gt_boxes: Optional[torch.Tensor], iou_match: float = 0.5, first_cam: int = 0) -> List[dict]:
    """One record per camera from dets [B,D,6] and gsr_det_verdict's best [B,4] (iou, score, class, row; -1: none): cam, pred_class,
    confidence, bbox, gt_bbox, iou -- the fields of the reference's per-camera log line (utils/render.py:280-289).  pred_class and
    confidence are those of the detection closest to the gt box when its IoU exceeds iou_match, else None; boxes are xywh rounded
    to 0.1.  One read-back."""
    B = int(dets.shape[0])
    row = best[:, 3].to(torch.int64).clamp(min=0)
    rows = dets[torch.arange(B, device=dets.device), row].cpu().tolist()
    best_h = best.cpu().tolist()
    gt_h = None if gt_boxes is None else torch.as_tensor(gt_boxes, dtype=torch.float32).cpu().tolist()
    out = []
    for v in range(B):
        iou, score, cls, r = best_h[v]
        has = r >= 0
        near = has and iou > iou_match
        gt = None if gt_h is None or any(x != x for x in gt_h[v]) else _xywh(gt_h[v])
        out.append(dict(cam=first_cam + v, pred_class=int(cls) if near else None, confidence=float(score) if near else None,
                        bbox=_xywh(rows[v][:4]) if has else None, gt_bbox=gt, iou=float(iou) if has else None))
    return out


@torch.no_grad()
def evaluate_views(model, background, cameras, detect: Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor]], *, target: int,
                   gt_boxes=None, benign=None, num_classes: int = 80, evaluator: Optional[DetectionEval] = None, bg_color=None, pipe=None,
                   iou_match: float = 0.5, batch: int = 8) -> Dict[str, object]:
    """The reference's evaluation sweep.  Every camera is rendered with `model` in front of `background` (a GaussianModel, joined
    by combine_with_background, or None: the model alone) through render_views; detect(images [B,3,H,W]) -> (dets [B,D,6], counts
    [B,2]) is the user's network plus one of the detector output stages; gsr_det_verdict and DetectionEval (default:
    reference_eval()) score it.  gt_boxes [V,4] (x1 y1 x2 y2, a NaN row: none; default: benign_bboxes of `model` alone on black, as
    the reference takes them) are annotated with class `target`.  benign: the unattacked model; given, the same sweep runs for it
    and the attack success rate compares the two.
    -> dict(metrics = compute()'s result, records = one per camera, verdict int32 [V], asr = (successful, total, rate) or None,
            dets, counts and, with `benign`, benign_metrics / benign_records / benign_verdict)."""
    from .attack import benign_bboxes, combine_with_background
    from .renderer import PipelineParams, render_views
    cams = list(cameras)
    if not cams:
        raise ValueError("evaluate_views: no cameras")
    dev = model.get_xyz.device
    pipe = pipe or PipelineParams()
    bg = torch.zeros(3, device=dev) if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32).to(dev)
    if gt_boxes is None:
        boxes = benign_bboxes(model, cams)
        gt_boxes = torch.tensor([[float("nan")] * 4 if b is None else [float(x) for x in b] for b in boxes], dtype=torch.float32)
    gt = torch.as_tensor(gt_boxes, dtype=torch.float32).to(dev)
    if tuple(gt.shape) != (len(cams), 4):
        raise ValueError(f"evaluate_views: gt_boxes must be [{len(cams)},4], got {tuple(gt.shape)}")
    gt_cls = torch.full((len(cams),), int(target), dtype=torch.int32, device=dev)

    def sweep(front, ev: DetectionEval):
        scene = front if background is None else combine_with_background(front, background)
        ev.reset()
        verdicts, records, all_dets, all_counts = [], [], [], []
        for i in range(0, len(cams), max(1, int(batch))):
            group = cams[i:i + max(1, int(batch))]
            images = torch.stack([r["render"] for r in render_views(group, scene, pipe, bg)]).clamp(0.0, 1.0)
            dets, counts = detect(images)
            sl = slice(i, i + len(group))
            ev.update(dets, counts, gt[sl], gt_cls[sl])
            bits, best = verdict_of(dets, counts, gt[sl], int(target), None, True, iou_match)
            verdicts.append(bits)
            records.extend(view_records(dets, best, gt[sl], iou_match, first_cam=i))
            all_dets.append(dets)
            all_counts.append(counts)
        return ev.compute(), records, torch.cat(verdicts), torch.cat(all_dets), torch.cat(all_counts)

    ev = evaluator or reference_eval(num_classes=num_classes)
    out: Dict[str, object] = {}
    if benign is not None:
        out["benign_metrics"], out["benign_records"], out["benign_verdict"], _, _ = sweep(benign, ev)
    out["metrics"], out["records"], out["verdict"], out["dets"], out["counts"] = sweep(model, ev)
    out["asr"] = attack_success_rate(out["benign_verdict"], out["verdict"]) if benign is not None else None
    return out


def to_coco_json(records: Sequence[dict], dets: torch.Tensor, counts: torch.Tensor, gt_path: str, dt_path: str, *, target: int,
                 width: int, height: int, categories: Optional[Dict[str, int]] = None) -> Tuple[int, int]:
    """The two files of utils/analyze_ap_ar.py:99-148 for a machine that has pycocotools: gt_path holds images (id = the record's
    cam), one annotation per record with a gt_bbox (category `target`, area w * h, iscrowd 0) and the categories (default: the
    target alone); dt_path holds EVERY detection row below counts[v,0] of dets [V,D,6] whose floats are finite and whose class is an
    integer -- image_id, category_id = the class, bbox xywh rounded to 0.1, score -- as utils/render.py:274-298 dumps them.
    -> (annotations, detections) written."""
    if len(records) != int(dets.shape[0]) or tuple(counts.shape) != (int(dets.shape[0]), 2):
        raise ValueError(f"to_coco_json: {len(records)} records, dets {tuple(dets.shape)}, counts {tuple(counts.shape)}")
    images, anns, res = [], [], []
    d, c = dets.detach().cpu().to(torch.float32).numpy(), counts.detach().cpu().numpy()
    for v, rec in enumerate(records):
        images.append(dict(id=int(rec["cam"]), width=int(width), height=int(height), file_name=""))
        if rec.get("gt_bbox"):
            b = [float(x) for x in rec["gt_bbox"]]
            anns.append(dict(id=len(anns) + 1, image_id=int(rec["cam"]), category_id=int(target), bbox=b, area=b[2] * b[3], iscrowd=0))
        for row in d[v, :min(max(int(c[v, 0]), 0), d.shape[1])]:
            if not np.isfinite(row).all() or row[5] != np.floor(row[5]) or row[5] < 0:
                continue
            res.append(dict(image_id=int(rec["cam"]), category_id=int(row[5]), bbox=_xywh(row[:4]), score=float(row[4])))
    cats = categories if categories is not None else {str(int(target)): int(target)}
    with open(gt_path, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=int(i), name=str(n)) for n, i in cats.items()]), f)
    with open(dt_path, "w") as f:
        json.dump(res, f)
    return len(anns), len(res)


def from_coco_json(gt_path: str, dt_path: str):
    """The two files back into the tensors update() takes, images in the order of the gt file's `images`: (dets float32 [N,D,6],
    counts int32 [N,2], gt_boxes float32 [N,M,4], gt_cls int32 [N,M], image_ids).  D and M are the largest per-image counts (at
    least 1 and 0); missing rows are zero detections beyond the count and ground truth of class -1.  Classes are the files'
    category ids; boxes come back as x1 y1 x2 y2 = x, y, x + w, y + h.  CPU tensors: move them to the device."""
    with open(gt_path) as f:
        gt = json.load(f)
    with open(dt_path) as f:
        dt = json.load(f)
    ids = [im["id"] for im in gt["images"]]
    at = {i: n for n, i in enumerate(ids)}
    per_gt: List[list] = [[] for _ in ids]
    per_dt: List[list] = [[] for _ in ids]
    for a in gt.get("annotations", ()):
        if not a.get("iscrowd", 0):
            per_gt[at[a["image_id"]]].append(a)
    for r in dt:
        per_dt[at[r["image_id"]]].append(r)
    N, D, M = len(ids), max([1] + [len(x) for x in per_dt]), max([0] + [len(x) for x in per_gt])
    dets, counts = torch.zeros((N, D, 6), dtype=torch.float32), torch.zeros((N, 2), dtype=torch.int32)
    gt_boxes, gt_cls = torch.zeros((N, M, 4), dtype=torch.float32), torch.full((N, M), -1, dtype=torch.int32)
    for n in range(N):
        for i, r in enumerate(per_dt[n]):
            x, y, w, h = r["bbox"]
            dets[n, i] = torch.tensor([x, y, x + w, y + h, r["score"], r["category_id"]], dtype=torch.float64).to(torch.float32)
        counts[n] = len(per_dt[n])
        for i, a in enumerate(per_gt[n]):
            x, y, w, h = a["bbox"]
            gt_boxes[n, i] = torch.tensor([x, y, x + w, y + h], dtype=torch.float64).to(torch.float32)
            gt_cls[n, i] = int(a["category_id"])
    return dets, counts, gt_boxes, gt_cls, ids

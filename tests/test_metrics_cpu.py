"""gsplat_attack.metrics, the parts that need no GPU: the attack success rate from verdict words, the record format, the COCO
JSON round trip, the evaluator's argument checks and CPU tensors raising (no fallback)."""
import json

import numpy as np
import pytest
import torch

import gsplat_attack
from gsplat_attack import metrics as MT


def test_attack_success_rate_counts_verdict_bits():
    # bit 1 (value 2) is target_exists; bits 0 and 2 do not matter
    benign = torch.tensor([7, 2, 6, 4, 0, 3, 2], dtype=torch.int32)
    adv = torch.tensor([7, 4, 0, 7, 2, 5, 6], dtype=torch.int32)
    # views whose benign prediction is the target: 0, 1, 2, 5, 6; of them the adversarial one is not: 1, 2, 5
    assert MT.attack_success_rate(benign, adv) == (3, 5, 0.6)
    assert MT.attack_success_rate([2, 2], [0, 0]) == (2, 2, 1.0)
    assert MT.attack_success_rate(np.array([6]), np.array([6])) == (0, 1, 0.0)
    assert MT.attack_success_rate([4, 0, 1], [0, 0, 0]) == (0, 0, 0.0)          # total 0: rate 0.0, not a division
    assert MT.attack_success_rate([], []) == (0, 0, 0.0)
    with pytest.raises(ValueError):
        MT.attack_success_rate([2, 2], [2])


def test_record_format():
    dets = torch.zeros(3, 4, 6)
    dets[0, 1] = torch.tensor([10.04, 20.06, 50.0, 80.26, 0.875, 2.0])
    dets[1, 0] = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.5, 1.0])
    best = torch.tensor([[0.75, 0.875, 2.0, 1.0], [0.25, 0.5, 1.0, 0.0], [-1.0, -1.0, -1.0, -1.0]])
    gt = torch.tensor([[10.0, 20.0, 50.0, 80.0], [0.0, 0.0, 9.96, 5.0], [float("nan")] * 4])
    r = MT.view_records(dets, best, gt, first_cam=5)
    assert [list(x) for x in r] == [["cam", "pred_class", "confidence", "bbox", "gt_bbox", "iou"]] * 3
    assert r[0] == dict(cam=5, pred_class=2, confidence=0.875, bbox=[10.0, 20.1, 40.0, 60.2], gt_bbox=[10.0, 20.0, 40.0, 60.0], iou=0.75)
    # the closest detection is below the match IoU: no class, no confidence, but its box and IoU are logged
    assert r[1] == dict(cam=6, pred_class=None, confidence=None, bbox=[1.0, 2.0, 2.0, 2.0], gt_bbox=[0.0, 0.0, 10.0, 5.0], iou=0.25)
    assert r[2] == dict(cam=7, pred_class=None, confidence=None, bbox=None, gt_bbox=None, iou=None)
    json.dumps(r)                                           # plain Python values


def test_coco_json_round_trip(tmp_path):
    g = torch.Generator().manual_seed(3)
    V, D = 4, 6
    xy = (torch.rand(V, D, 2, generator=g) * 100).round(decimals=1)
    wh = (torch.rand(V, D, 2, generator=g) * 50 + 1).round(decimals=1)
    dets = torch.cat([xy, xy + wh, torch.rand(V, D, 1, generator=g), torch.randint(0, 5, (V, D, 1), generator=g).float()], -1)
    counts = torch.tensor([[6, 6], [3, 9], [0, 0], [1, 1]], dtype=torch.int32)
    dets[1, 1, 4] = float("nan")                            # a dead row is not written
    gt = torch.tensor([[10.0, 10.0, 60.0, 40.0], [5.5, 6.5, 20.0, 30.0], [float("nan")] * 4, [0.0, 0.0, 8.0, 8.0]])
    best = torch.full((V, 4), -1.0)
    records = MT.view_records(dets, best, gt, first_cam=10)
    gp, dp = str(tmp_path / "gt.json"), str(tmp_path / "preds.json")
    assert MT.to_coco_json(records, dets, counts, gp, dp, target=2, width=640, height=480) == (3, 6 + 2 + 0 + 1)
    gj, dj = json.load(open(gp)), json.load(open(dp))
    assert sorted(gj) == ["annotations", "categories", "images"] and gj["categories"] == [dict(id=2, name="2")]
    assert gj["images"][0] == dict(id=10, width=640, height=480, file_name="") and [i["id"] for i in gj["images"]] == [10, 11, 12, 13]
    assert gj["annotations"][1] == dict(id=2, image_id=11, category_id=2, bbox=[5.5, 6.5, 14.5, 23.5], area=14.5 * 23.5, iscrowd=0)
    assert sorted(dj[0]) == ["bbox", "category_id", "image_id", "score"] and dj[0]["image_id"] == 10
    d2, c2, gb2, gc2, ids = MT.from_coco_json(gp, dp)
    assert ids == [10, 11, 12, 13] and c2.tolist() == [[6, 6], [2, 2], [0, 0], [1, 1]]
    assert tuple(d2.shape) == (V, 6, 6) and tuple(gb2.shape) == (V, 1, 4) and gc2.tolist() == [[2], [2], [-1], [2]]
    assert torch.equal(d2[0, :, 4:], dets[0, :, 4:]) and torch.equal(d2[1, :2, 4:], dets[1, [0, 2], 4:])     # scores and classes exactly
    assert torch.allclose(d2[0, :, :4], dets[0, :, :4], atol=0.051) and torch.allclose(gb2[1, 0], gt[1], atol=1e-5)
    assert (d2[2] == 0).all() and (d2[1, 2:] == 0).all()
    # a second trip changes nothing: the files hold one decimal
    r2 = MT.view_records(d2, best, gb2[:, 0], first_cam=10)
    r2[2]["gt_bbox"] = None
    g2, p2 = str(tmp_path / "gt2.json"), str(tmp_path / "preds2.json")
    MT.to_coco_json(r2, d2, c2, g2, p2, target=2, width=640, height=480)
    d3, c3, gb3, gc3, _ = MT.from_coco_json(g2, p2)
    assert torch.equal(c3, c2) and torch.allclose(d3, d2, atol=1e-4) and torch.equal(gc3[[0, 1, 3]], gc2[[0, 1, 3]])
    with pytest.raises(ValueError):
        MT.to_coco_json(records[:2], dets, counts, gp, dp, target=2, width=1, height=1)


def test_evaluator_checks_and_cpu_tensors_raise():
    ev = MT.DetectionEval(80)
    assert ev.iou_thrs.dtype == np.float64 and np.array_equal(ev.iou_thrs, np.linspace(0.5, 0.95, 10))
    assert np.array_equal(ev.rec_thrs, np.linspace(0.0, 1.0, 101)) and ev.max_dets == (1, 10, 100)
    assert ev.area_ranges == ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10)) and ev.num_images == 0
    assert ev.spec(300).max_dets == (1, 10, 100) and ev.spec(20).max_dets == (1, 10, 20) and ev.spec(5).max_dets == (1, 5, 5)
    assert ev.spec(300).n_rec == 101 and ev.spec(300).num_classes == 80
    ref = MT.reference_eval()
    assert ref.iou_thrs.tolist() == [0.5] and ref.num_classes == 80 and MT.reference_eval(0.75, 3).iou_thrs.tolist() == [0.75]
    for bad in (dict(num_classes=0), dict(num_classes=65536), dict(num_classes=3, iou_thrs=[0.5] * 11), dict(num_classes=3, iou_thrs=[]),
                dict(num_classes=3, rec_thrs=np.zeros(1025)), dict(num_classes=3, area_ranges=((0, 1),) * 5), dict(num_classes=3, max_dets=(1, 2, 3, 4)),
                dict(num_classes=3, max_dets=(10, 1)), dict(num_classes=3, max_dets=(0, 1)), dict(num_classes=3, max_dets=())):
        with pytest.raises(ValueError):
            MT.DetectionEval(**bad)
    dets, counts = torch.zeros(2, 100, 6), torch.zeros(2, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.update(dets, counts, torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ev.update(torch.zeros(2, 100, 5), counts, torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no update"):
        ev.compute()
    for name in ("DetectionEval", "reference_eval", "attack_success_rate", "evaluate_views", "to_coco_json", "from_coco_json"):
        assert getattr(gsplat_attack, name) is getattr(MT, name)

"""The detection metrics' kernels on the GPU (gsr_deteval_match / _accumulate / _summarize) against the float64 oracle of
tests/deteval_cases.py: every integer output equal, every double bit for bit, on every case; two runs bit for bit; recall
thresholds as the caller passes them; DetectionEval in one batch against three; evaluate_views on hydrant-1k with a stub detector
whose outputs are constructed; and the dets of the three detector output stages accepted as they come."""
import numpy as np
import pytest
import torch

import deteval_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _eval_spec(spec, n_rec=None):
    from diff_gaussian_rasterization import deteval_ops as EO
    return EO.EvalSpec(spec.K, tuple(spec.iou.tolist()), spec.areas, spec.caps, spec.R if n_rec is None else n_rec)


def gpu_run(spec, batches, dev, rec_thrs=None):
    from diff_gaussian_rasterization import deteval_ops as EO
    rec = np.ascontiguousarray(spec.rec if rec_thrs is None else rec_thrs, np.float64)
    es = _eval_spec(spec, len(rec))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ms = [EO.match(t(d), t(c), t(g), t(k), es) for d, c, g, k in batches]
    m = EO.MatchOut(*(torch.cat([getattr(x, f) for x in ms]) for f in EO.MatchOut._fields))
    dets = t(np.concatenate([b[0] for b in batches]))
    gt_cls = t(np.concatenate([b[3] for b in batches]))
    precision, scores, recall, npig = EO.accumulate(dets, m, gt_cls, t(rec), es)
    stats = EO.summarize(precision, recall, es)
    out = dict(zip(EO.MatchOut._fields, m))
    out.update(precision=precision, scores=scores, recall=recall, npig=npig, stats=stats)
    return out


@pytest.mark.parametrize("name", DC.ALL)
def test_kernels_match_oracle(dev, name):
    spec, batches = DC.case(name)
    DC.check(f"gpu {name}", gpu_run(spec, batches, dev), DC.oracle(name))


def test_literal_numbers(dev):
    spec, batches = DC.literal()
    got = gpu_run(spec, batches, dev)
    p = got["precision"].cpu().numpy()[0, :, 0, 0, 0]
    one = 1 / (1 + DC.EPS)                                    # COCOeval's precision of a lone true positive: the double below 1
    assert one < 1.0 and (p[:34] == one).all() and DC.same(p[34:67], np.full(33, 2 / (3 + DC.EPS))) and (p[67:] == 0.0).all()
    st = got["stats"].cpu().numpy()
    assert abs(st[0] - 56 / 101) <= 101 * 2.0 ** -52 and st[8] == -1.0 and st[12] == st[0] and st[13] == st[6] == 2 / 3


@pytest.mark.parametrize("name", ["T10-batches", "counts-D129", "scan-carry"])
def test_two_runs_bit_for_bit(dev, name):
    spec, batches = DC.case(name)
    a, b = gpu_run(spec, batches, dev), gpu_run(spec, batches, dev)
    for k in a:
        assert DC.same(a[k].cpu().numpy(), b[k].cpu().numpy()), k


def test_recall_thresholds_are_the_callers(dev):
    """tp / 100 meets thresholds where numpy.linspace(0, 1, 101)[i] and i / 100.0 differ in the last bit: each array gives its own
    oracle's result"""
    spec, batches = DC.case("recall-100")
    lin, div = np.linspace(0.0, 1.0, 101), np.arange(101) / 100.0
    assert (lin != div).any()
    outs = []
    for rec in (lin, div):
        ref = DC.oracle_run(spec, batches, rec)
        got = gpu_run(spec, batches, dev, rec)
        DC.check("gpu recall-100", got, ref)
        outs.append(ref["precision"])
    assert not DC.same(outs[0], outs[1])                       # the case tells the two arrays apart


def test_update_in_one_batch_and_in_three(dev):
    from gsplat_attack.metrics import DetectionEval
    spec, batches = DC.case("T10-batches")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ev = DetectionEval(spec.K, max_dets=spec.caps)
    for d, c, g, k in batches:
        ev.update(t(d), t(c), t(g), t(k))
    three = ev.compute()
    ev.reset()
    assert ev.num_images == 0
    ev.update(*(t(np.concatenate([b[i] for b in batches])) for i in range(4)))
    one = ev.compute()
    ref = DC.oracle("T10-batches")
    for k in DC.ACC_KEYS:
        assert DC.same(three[k].cpu().numpy(), one[k].cpu().numpy()) and DC.same(one[k].cpu().numpy(), ref[k]), k
    assert list(one["stats"]) == list(DC.STAT_NAMES)
    assert DC.same(np.array(list(one["stats"].values())), ref["stats"]) and one["stats"] == three["stats"]
    # ... and against numpy.mean over the same slices, within n 2^-52 (pairwise against sequential summation of values in [0, 1])
    for name, sl in zip(DC.STAT_NAMES, DC.stat_slices(spec, ref["precision"], ref["recall"])):
        v = sl[sl > -1]
        assert abs(one["stats"][name] - (np.mean(v) if v.size else -1.0)) <= max(v.size, 1) * 2.0 ** -52, name


def test_batches_of_unequal_gt_rows_and_caps_above_D(dev):
    """update() with M = 3 and then M = 1 (absent rows are padded behind), caps (1, 10, 100) with D = 12: the caps D admits"""
    from gsplat_attack.metrics import DetectionEval
    spec, batches = DC.case("empty-classes")
    d, c, g, k = batches[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    g2, k2 = g.copy(), k.copy()
    k2[1, 1:] = -1                                             # image 1 keeps its first row only
    ev = DetectionEval(spec.K)
    ev.update(t(d[:1]), t(c[:1]), t(g2[:1]), t(k2[:1]))
    ev.update(t(d[1:]), t(c[1:]), t(g2[1:, :1]), t(k2[1:, :1]))
    got = ev.compute()
    ref = DC.oracle_run(spec.replace(max_dets=(1, 10, 12)), [(d, c, g2, k2)])
    for key in DC.ACC_KEYS:
        assert DC.same(got[key].cpu().numpy(), ref[key]), key
    assert DC.same(got["stats_tensor"].cpu().numpy(), ref["stats"])


def test_evaluate_views_on_hydrant(dev):
    from gsplat_attack.metrics import evaluate_views, reference_eval
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=dev, n_views=4)
    back, _, _ = make_scene("hydrant-1k", device=dev, n_views=1)
    V, D, K, target = 4, 5, 4, 2
    gt = np.array([[10, 12, 50, 60], [20, 20, 70, 90], [5, 5, 40, 30], [np.nan] * 4], np.float32)
    adv = np.zeros((V, D, 6), np.float32)
    ben = np.zeros((V, D, 6), np.float32)
    for v in range(3):
        ben[v, 0] = (*gt[v], 0.9, target)                      # the benign sweep sees the target on its box in views 0..2
    ben[3, 0] = (1, 1, 9, 9, 0.8, target)                      # no gt box: the class alone decides
    adv[0, 0] = (*gt[0], 0.85, target)                         # view 0: still the target
    adv[0, 1] = (100, 100, 120, 130, 0.95, 1)
    adv[1, 0] = (*gt[1], 0.7, 1)                               # view 1: another class on the box
    adv[1, 1] = (21, 20, 70, 90, 0.6, target)                  # ... and the target a little off it, at a lower IoU
    adv[3, 0] = (1, 1, 9, 9, 0.8, 3)                           # view 2: no detections at all; view 3 (no gt box): another class
    n_ben, n_adv = np.array([[1, 1]] * 4, np.int32), np.array([[2, 2], [2, 2], [0, 0], [1, 1]], np.int32)
    seen = []

    def detect(images):                                        # the renders decide nothing here: the outputs are constructed
        assert images.shape[1] == 3 and images.is_cuda and float(images.min()) >= 0.0 and float(images.max()) <= 1.0
        first = sum(seen) % V
        src, cnt = (ben, n_ben) if sum(seen) < V else (adv, n_adv)
        seen.append(int(images.shape[0]))
        sl = slice(first, first + images.shape[0])
        return torch.from_numpy(src[sl]).to(dev), torch.from_numpy(cnt[sl]).to(dev)

    out = evaluate_views(model, back, cams, detect, target=target, gt_boxes=gt, benign=model, num_classes=K, batch=3)
    assert seen == [3, 1, 3, 1]
    assert out["asr"] == (3, 4, 0.75)                           # views 1, 2 and 3 lose the target, view 0 keeps it
    assert out["verdict"].cpu().tolist() == [3 | 4, 4, 4, 4] and out["benign_verdict"].cpu().tolist() == [7, 7, 7, 7]
    spec = DC.Spec(K, D, 1, iou_thrs=[0.5])
    gcls = np.where(np.isnan(gt).any(1), -1, target).astype(np.int32)[:, None]
    for key, src, cnt in (("metrics", adv, n_adv), ("benign_metrics", ben, n_ben)):
        ref = DC.oracle_run(spec.replace(max_dets=(1, 5, 5)), [(src, cnt, np.nan_to_num(gt)[:, None, :], gcls)])
        for k in DC.ACC_KEYS:
            assert DC.same(out[key][k].cpu().numpy(), ref[k]), (key, k)
        assert DC.same(np.array(list(out[key]["stats"].values())), ref["stats"])
    assert out["benign_metrics"]["stats"]["ap_ref"] == 1.0 and out["benign_metrics"]["stats"]["ar_ref"] == 1.0
    r = out["records"]
    assert [x["cam"] for x in r] == [0, 1, 2, 3]
    assert r[0] == dict(cam=0, pred_class=target, confidence=pytest.approx(0.85), bbox=[10.0, 12.0, 40.0, 48.0], gt_bbox=[10.0, 12.0, 40.0, 48.0], iou=1.0)
    assert r[1]["pred_class"] == 1 and r[1]["bbox"] == [20.0, 20.0, 50.0, 70.0] and r[1]["iou"] == 1.0
    assert r[2] == dict(cam=2, pred_class=None, confidence=None, bbox=None, gt_bbox=[5.0, 5.0, 35.0, 25.0], iou=None)
    assert r[3]["gt_bbox"] is None and r[3]["pred_class"] is None and r[3]["bbox"] is None
    assert torch.equal(out["dets"].cpu(), torch.from_numpy(adv)) and torch.equal(out["counts"].cpu(), torch.from_numpy(n_adv))
    assert isinstance(reference_eval(0.75).iou_thrs, np.ndarray) and reference_eval(0.75).iou_thrs.tolist() == [0.75]


def test_detector_stage_outputs_are_accepted(dev):
    """the dets / counts of gsr_det_postprocess, gsr_setdet_postprocess (query order: the sort works) and gsr_rcnn_postprocess,
    as they come, against the oracle on the same arrays"""
    from diff_gaussian_rasterization import detect_ops, rcnn_ops, setdet_ops
    from gsplat_attack.metrics import DetectionEval
    g = torch.Generator().manual_seed(5)
    B, A, C = 3, 200, 3
    gt = torch.tensor([[[20., 20., 90., 100.], [100., 40., 140., 90.]]] * B)
    gt_cls = torch.tensor([[0, 2]] * B, dtype=torch.int32)
    outs = {}
    # YOLO-style head [B,A,4+C], boxes (xc, yc, w, h) near the gt rows
    ctr = torch.tensor([55., 60., 70., 80.]) + 6 * torch.randn(B, A, 4, generator=g)
    raw = torch.cat([ctr, torch.rand(B, A, C, generator=g)], -1)
    outs["det"] = detect_ops.postprocess(raw.to(dev), detect_ops.DetSpec(layout=0, conf_thr=0.3, iou_thr=0.6, max_det=40))
    # set-prediction head: logits [B,Q,C+1], boxes (cx, cy, w, h) normalised
    Q = 30
    logits = 3 * torch.randn(B, Q, C + 1, generator=g)
    boxes = (torch.tensor([0.3, 0.3, 0.35, 0.4]) + 0.03 * torch.randn(B, Q, 4, generator=g)).clamp(0.05, 0.9)
    outs["setdet"] = setdet_ops.postprocess(logits.to(dev), boxes.to(dev), setdet_ops.SetDetSpec(img_w=200., img_h=200., conf_thr=0.3))
    # box head: scores [B,R,C+1], class-specific deltas, proposals
    R = 60
    props = torch.tensor([20., 20., 90., 100.]) + 5 * torch.randn(B, R, 4, generator=g)
    sc = 2 * torch.randn(B, R, C + 1, generator=g)
    dl = 0.1 * torch.randn(B, R, 4 * C, generator=g)
    outs["rcnn"] = rcnn_ops.postprocess(sc.to(dev), dl.to(dev), props.to(dev), rcnn_ops.RcnnSpec(conf_thr=0.2, img_w=200., img_h=200., max_det=25))
    for name, (dets, counts) in outs.items():
        D = int(dets.shape[1])
        assert int(counts[:, 0].min()) >= 2, (name, counts.cpu().tolist())
        ev = DetectionEval(C, max_dets=(1, 10, D))
        ev.update(dets, counts, gt.to(dev), gt_cls.to(dev))
        got = ev.compute()
        spec = DC.Spec(C, D, 2, max_dets=(1, min(10, D), D))
        ref = DC.oracle_run(spec, [(dets.cpu().numpy(), counts.cpu().numpy(), gt.numpy(), gt_cls.numpy())])
        for k in DC.ACC_KEYS:
            assert DC.same(got[k].cpu().numpy(), ref[k]), (name, k)
        assert DC.same(got["stats_tensor"].cpu().numpy(), ref["stats"]), name
        if name == "setdet":                                   # query order is not score order
            s = dets[0, :int(counts[0, 0]), 4].cpu()
            assert not bool((s[:-1] >= s[1:]).all())

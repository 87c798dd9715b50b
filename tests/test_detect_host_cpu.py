"""The detector output stage's arithmetic on the CPU: csrc/gsr_detect.h compiled by g++ (tests/host_math/detect_host.cpp)
against the numpy oracle of tests/detect_cases.py, which is written from the contract with float64 IoUs.  Kept anchors,
classes, counts and verdict bits are integer-equal; boxes and scores are bit-equal (they are copies of inputs, or the
contract's exactly specified float32 operations on them).  The GPU tests then require the kernels to equal this host
build bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import detect_cases as DC
from detect_cases import F32, Case

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return DC.host_lib()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("c", DC.CASES, ids=lambda c: c.id)
def test_postprocess_and_verdict_against_the_oracle(lib, c):
    pred, dets, counts, gap = DC.reference(c)
    # the condition under which float32 and float64 must agree (module doc of detect_cases): asserted, never skipped
    assert gap > DC.MARGIN, f"seed {c.seed}: a candidate pair's IoU lies {gap:.2e} from iou_thr"
    hd, hc = DC.host_postprocess(lib, c, pred)
    assert np.array_equal(hc, counts)
    assert _same(hd, dets)                          # boxes, scores, classes and the zero rows, bit for bit
    gt = DC.make_gt(c, dets, counts)
    if c.B > 1:
        gt[0] = NAN                                 # one image without a gt box
    for target, untarget, targeted in ((0, 1, True), (1, None, True), (2, 0, False), (0, None, False)):
        bits, best, vgap = DC.oracle_verdict(dets, counts, gt, target, untarget, targeted, 0.5)
        assert vgap > DC.MARGIN, f"seed {c.seed}: a det-gt IoU lies {vgap:.2e} from iou_match"
        hb, hbest = DC.host_verdict(lib, hd, hc, gt, target, untarget, targeted, 0.5)
        assert np.array_equal(hb, bits)
        assert np.array_equal(hbest[:, 1:], best[:, 1:].astype(F32))           # score, class, row
        assert np.abs(hbest[:, 0].astype(np.float64) - best[:, 0]).max() <= 1e-6
    bits, _, _ = DC.oracle_verdict(dets, counts, None, 0, 1, True, 0.5)         # no gt at all
    assert np.array_equal(DC.host_verdict(lib, hd, hc, None, 0, 1, True, 0.5)[0], bits)


def test_the_cases_cover_what_they_claim():
    by_id = {c.id: DC.reference(c) for c in DC.CASES}
    counts = [v[2] for v in by_id.values()]
    assert any((c[:, 1] > 4096).any() for c in counts)                          # more than max_candidates above the threshold
    assert any((c[:, 0] == 0).any() and (c[:, 0] > 0).any() for c in counts)    # an image with none next to images with some
    assert any(c.max_det == 20 and r[2][0, 0] == 20 for c, r in zip(DC.CASES, by_id.values()))   # survivors cut at max_det
    aware, agnostic = (DC.reference(c)[2][0, 0] for c in DC.CASES if c.A == 1025)
    assert agnostic < aware                          # the same boxes: the class compare spares boxes
    over = next(c for c in DC.CASES if c.maxc == 256)
    pred = DC.reference(over)[0]
    score, _ = DC.oracle_scores(over, pred)
    order = DC.order_of(score[0], np.nonzero(score[0] > F32(over.conf))[0])
    assert score[0, order[255]] == score[0, order[256]]                         # tied scores at the cut: the anchor index decides


@pytest.mark.parametrize("n,n_valid", [(1, None), (65, (40,)), (300, None), (700, (700, 0, 129))])
def test_nms_entry_against_the_oracle(lib, n, n_valid):
    B = 1 if n_valid is None else len(n_valid)
    for seed in range(50):                           # the first seed that meets the margin condition; it is then asserted
        rng = np.random.default_rng(900 + n + 31 * seed)
        boxes = np.stack([DC.make_boxes(rng, n, 5) for _ in range(B)])
        scores = (np.round(rng.uniform(0, 1, (B, n)) * 128) / 128).astype(F32)
        classes = rng.integers(0, 3, (B, n)).astype(np.int32)
        nv = None if n_valid is None else np.asarray(n_valid, np.int32)
        max_det = min(n, 40)
        keep, counts, gap = DC.oracle_nms(boxes, scores, classes, nv, 0.45, max_det)
        if gap > DC.MARGIN:
            break
    assert gap > DC.MARGIN
    hk, hc = DC.host_nms(lib, boxes, scores, classes, nv, 0.45, max_det)
    assert np.array_equal(hk, keep) and np.array_equal(hc, counts)
    keep_a, counts_a, _ = DC.oracle_nms(boxes, scores, None, nv, 0.45, max_det)
    hk, hc = DC.host_nms(lib, boxes, scores, None, nv, 0.45, max_det)
    assert np.array_equal(hk, keep_a) and np.array_equal(hc, counts_a)


@pytest.mark.parametrize("n,m", [(1, 1), (65, 3), (300, 1)])
def test_box_iou_against_float64(lib, n, m):
    rng = np.random.default_rng(n * 7 + m)
    a, b = DC.make_boxes(rng, n, 2), DC.make_boxes(rng, m, 2)
    got = DC.host_box_iou(lib, a, b)
    want = DC.oracle_box_iou(a, b)
    # coordinates <= 2000 px: a handful of float32 roundings, each 2^-24 relative, on a value <= 1
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-6


# ---- hand-made exact cases ----------------------------------------------------------------------------------------------
def _nms(lib, boxes, scores, thr, classes=None, max_det=None):
    boxes = np.asarray(boxes, F32)[None]
    scores = np.asarray(scores, F32)[None]
    cl = None if classes is None else np.asarray(classes, np.int32)[None]
    keep, counts = DC.host_nms(lib, boxes, scores, cl, None, thr, max_det or boxes.shape[1])
    return keep[0, :counts[0]].tolist()


def test_iou_exactly_at_the_threshold_is_not_suppressed(lib):
    boxes = [[0, 0, 3, 1], [1, 0, 4, 1]]             # inter 2, union 4: IoU exactly 0.5
    assert DC.host_box_iou(lib, np.asarray(boxes[:1], F32), np.asarray(boxes[1:], F32))[0, 0] == F32(0.5)
    assert _nms(lib, boxes, [0.9, 0.8], 0.5) == [0, 1]
    below = float(np.nextafter(F32(0.5), F32(0)))
    assert _nms(lib, boxes, [0.9, 0.8], below) == [0]
    assert _nms(lib, boxes, [0.8, 0.9], below) == [1]


def test_identical_boxes_and_class_compare(lib):
    boxes = [[10, 10, 50, 60]] * 3
    assert _nms(lib, boxes, [0.5, 0.7, 0.6], 0.45) == [1]
    assert _nms(lib, boxes, [0.5, 0.7, 0.6], 0.45, classes=[0, 1, 0]) == [1, 2]
    assert _nms(lib, boxes, [0.5, 0.7, 0.6], 0.45, classes=[0, 1, 2]) == [1, 2, 0]
    # all boxes suppressed by the first
    many = [[100 + 0.01 * i, 100, 200, 200] for i in range(130)]
    assert _nms(lib, many, list(np.linspace(0.9, 0.1, 130)), 0.45) == [0]


def test_zero_area_boxes_give_nan_and_are_both_kept(lib):
    boxes = [[5, 5, 5, 5], [5, 5, 5, 5]]
    assert np.isnan(DC.host_box_iou(lib, np.asarray(boxes, F32), np.asarray(boxes, F32))).all()
    assert _nms(lib, boxes, [0.9, 0.8], 0.0) == [0, 1]


def test_equal_scores_walk_in_anchor_order(lib):
    boxes = [[0, 0, 10, 10], [100, 0, 110, 10], [200, 0, 210, 10], [300, 0, 310, 10]]
    assert _nms(lib, boxes, [0.5, 0.75, 0.5, 0.75], 0.45) == [1, 3, 0, 2]
    assert _nms(lib, boxes, [0.0, -0.0, 0.0, -0.0], 0.45) == [0, 1, 2, 3]       # -0 and +0 are one score
    assert _nms(lib, boxes, [0.5, 0.75, 0.5, 0.75], 0.45, max_det=3) == [1, 3, 0]


def _one_class(scores, conf, **kw):
    """A = len(scores) far-apart boxes with one class each: which anchors come out, in order."""
    A = len(scores)
    c = Case(A, C=1, layout=0, box_format=1, conf=conf, **kw)
    pred = np.zeros((1, A, 5), F32)
    for a in range(A):
        pred[0, a, :4] = [100 * a, 0, 100 * a + 10, 10]
    pred[0, :, 4] = np.asarray(scores, F32)
    return c, pred


def test_threshold_nan_and_inf_scores(lib):
    conf = F32(0.7)
    up = np.nextafter(conf, F32(1))
    c, pred = _one_class([conf, up, NAN, INF, 0.1, -INF], float(conf))
    dets, counts = DC.host_postprocess(lib, c, pred)
    assert counts.tolist() == [[2, 2]]               # at the threshold: dropped; the next float above: kept; NaN: dropped
    assert dets[0, :2, 0].tolist() == [300.0, 100.0]                            # +inf first
    assert dets[0, 0, 4] == np.inf and _same(dets[0, 1, 4], up)
    assert not dets[0, 2:].any()
    od, oc, _ = DC.oracle_postprocess(c, pred)
    assert np.array_equal(oc, counts) and _same(od, dets)


def test_class_ties_nan_classes_and_objectness(lib):
    # anchor 0: classes tie -> the lowest index; anchor 1: a NaN class score never wins; anchor 2: every class NaN -> no candidate
    c = Case(3, C=3, layout=1, has_obj=True, box_format=1, conf=0.2)
    pred = np.zeros((1, 8, 3), F32)
    pred[0, :4] = np.asarray([[0, 100, 200], [0, 0, 0], [10, 110, 210], [10, 10, 10]], F32)
    pred[0, 4] = [0.5, 1.0, 1.0]
    pred[0, 5:, 0] = [0.25, 0.75, 0.75]          # the three class scores of anchor 0, then of anchors 1 and 2
    pred[0, 5:, 1] = [NAN, 0.5, 0.25]
    pred[0, 5:, 2] = [NAN, NAN, NAN]
    dets, counts = DC.host_postprocess(lib, c, pred)
    assert counts.tolist() == [[2, 2]]
    assert dets[0, 0].tolist() == [100.0, 0.0, 110.0, 10.0, 0.5, 1.0]
    assert dets[0, 1].tolist() == [0.0, 0.0, 10.0, 10.0, 0.375, 1.0]            # obj 0.5 * cls 0.75, the first of the tie
    od, oc, _ = DC.oracle_postprocess(c, pred)
    assert np.array_equal(oc, counts) and _same(od, dets)


def test_cap_keeps_the_first_of_the_order(lib):
    c, pred = _one_class([0.5, 0.75, 0.5, 0.75, 0.5], 0.25, maxc=3, max_det=3)
    dets, counts = DC.host_postprocess(lib, c, pred)
    assert counts.tolist() == [[3, 5]]
    assert dets[0, :, 0].tolist() == [100.0, 300.0, 0.0]


def test_verdict_modes_by_hand(lib):
    # row 0: class 2 at IoU exactly 0.5 with the gt (not a match at iou_match = 0.5); row 1: class 7, far away
    dets = np.zeros((4, 3, 6), F32)
    dets[:, 0] = [0, 0, 3, 1, 0.9, 2]
    dets[:, 1] = [50, 50, 60, 60, 0.8, 7]
    counts = np.asarray([[2, 2], [2, 2], [2, 2], [0, 0]], np.int32)
    gt = np.asarray([[1, 0, 4, 1], [NAN, 0, 4, 1], [0, 0, 3, 1], [1, 0, 4, 1]], F32)
    bits, best = DC.host_verdict(lib, dets, counts, gt, 2, 7, True, 0.5)
    #  image 0: best IoU == iou_match: no match, so no target, and the untarget is absent
    #  image 1: no gt (NaN row): class 2 is there, class 7 too
    #  image 2: IoU 1 with class 2
    #  image 3: no detections
    assert bits.tolist() == [4, 2, 7, 4]
    assert best.tolist() == [[0.5, F32(0.9), 2.0, 0.0], [-1.0] * 4, [1.0, F32(0.9), 2.0, 0.0], [-1.0] * 4]
    assert DC.host_verdict(lib, dets, counts, gt, 2, None, True, 0.5)[0].tolist() == [4, 7, 7, 4]
    assert DC.host_verdict(lib, dets, counts, gt, 2, 7, False, 0.5)[0].tolist() == [5, 2, 7, 5]
    assert DC.host_verdict(lib, dets, counts, gt, 2, 2, False, 0.5)[0].tolist() == [5, 2, 2, 5]
    below = float(np.nextafter(F32(0.5), F32(0)))
    assert DC.host_verdict(lib, dets, counts, gt, 2, 7, True, below)[0].tolist() == [7, 2, 7, 4]
    for args in ((2, 7, True), (2, None, True), (2, 7, False), (2, 2, False)):
        assert np.array_equal(DC.host_verdict(lib, dets, counts, gt, *args, 0.5)[0],
                              DC.oracle_verdict(dets, counts, gt, *args, 0.5)[0])


def test_score_key_is_monotone(lib):
    vals = np.asarray([-INF, -3.5, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.7, np.nextafter(F32(0.7), F32(1)), 1.0, INF], F32)
    keys = [lib.dh_score_key(float(v)) for v in vals]
    assert keys[3] == keys[4]
    assert keys[:4] == sorted(set(keys[:4])) and keys[4:] == sorted(set(keys[4:]))


def test_sanitized_harness(tmp_path):
    """tests/host_math/detect_harness.cpp: its own main over small exact-size buffers, built with AddressSanitizer and
    UBSan and run as a program."""
    exe = str(tmp_path / "detect_harness")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", DC.CSRC, os.path.join(DC.HM, "detect_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("detect_harness ok"), r.stdout + r.stderr

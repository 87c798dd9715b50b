"""The detector output stage on the device: every entry bit for bit the host build of the same source
(tests/host_math/detect_host.cpp, itself integer- and bit-equal to the numpy oracle: tests/test_detect_host_cpu.py, on
the very cases used here), on a non-default stream, twice in a row, and end to end behind a small torch head."""
import numpy as np
import pytest
import torch

import detect_cases as DC
from detect_cases import F32, Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(scope="module")
def host():
    return DC.host_lib()


@pytest.fixture(scope="module")
def DO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import detect_ops
    D._load()
    assert detect_ops.available()
    return detect_ops


def _spec(DO, c: Case):
    return DO.DetSpec(c.layout, c.has_obj, c.box_format, c.conf, c.iou, c.maxc, c.max_det, c.agnostic, *c.affine)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("c", DC.CASES, ids=lambda c: c.id)
def test_postprocess_and_verdict_bit_for_bit_the_host_build(host, DO, c):
    pred = DC.reference(c)[0]
    want_d, want_c = DC.host_postprocess(host, c, pred)
    x = torch.tensor(pred, device=DEV)
    dets, counts = DO.postprocess(x, _spec(DO, c))
    assert np.array_equal(_np(counts), want_c)
    assert np.array_equal(_bits(dets), _bits(want_d))
    again_d, again_c = DO.postprocess(x, _spec(DO, c))           # twice in a row: the same bits
    assert torch.equal(again_c, counts) and np.array_equal(_bits(again_d), _bits(dets))
    gt = DC.make_gt(c, want_d, want_c)
    if c.B > 1:
        gt[0] = NAN
    g = torch.from_numpy(gt).to(DEV)
    for target, untarget, targeted in ((0, 1, True), (1, None, True), (2, 0, False), (0, None, False)):
        for gt_np, gt_dev in ((gt, g), (None, None)):
            hb, hbest = DC.host_verdict(host, want_d, want_c, gt_np, target, untarget, targeted, 0.5)
            bits, best = DO.verdict(dets, counts, gt_dev, target, untarget, targeted, 0.5)
            assert np.array_equal(_np(bits), hb)
            assert np.array_equal(_bits(best), _bits(hbest))


def test_non_default_stream(host, DO):
    c = DC.CASES[4]
    pred = DC.reference(c)[0]
    want_d, want_c = DC.host_postprocess(host, c, pred)
    x = torch.tensor(pred, device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        dets, counts = DO.postprocess(x, _spec(DO, c))
        bits, best = DO.verdict(dets, counts, None, 0, 1, True, 0.5)
    s.synchronize()
    assert np.array_equal(_np(counts), want_c) and np.array_equal(_bits(dets), _bits(want_d))
    hb, hbest = DC.host_verdict(host, want_d, want_c, None, 0, 1, True, 0.5)
    assert np.array_equal(_np(bits), hb) and np.array_equal(_bits(best), _bits(hbest))


def _nms_inputs(n, B, seed):
    rng = np.random.default_rng(300 + n + seed)
    boxes = np.stack([DC.make_boxes(rng, n, 6) for _ in range(B)])
    scores = (np.round(rng.uniform(0, 1, (B, n)) * 128) / 128).astype(F32)
    classes = rng.integers(0, 3, (B, n)).astype(np.int32)
    return boxes, scores, classes


@pytest.mark.parametrize("n,n_valid,max_det", [(1, None, 1), (65, (40,), 65), (700, (700, 0, 129), 50), (4096, (4096, 513), 300)])
def test_nms_entry_bit_for_bit_the_host_build(host, DO, n, n_valid, max_det):
    B = 1 if n_valid is None else len(n_valid)
    boxes, scores, classes = _nms_inputs(n, B, 0)
    nv = None if n_valid is None else np.asarray(n_valid, np.int32)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    for cl in (classes, None):                       # class-aware and agnostic on the same boxes
        want_k, want_c = DC.host_nms(host, boxes, scores, cl, nv, 0.45, max_det)
        keep, counts = DO.nms(dev(boxes), dev(scores), 0.45, max_det, classes=dev(cl), n_valid=dev(nv))
        assert np.array_equal(_np(counts), want_c) and np.array_equal(_np(keep), want_k)
        assert (want_c <= max_det).all()


def test_nms_exact_cases(host, DO):
    def run(boxes, scores, thr, classes=None):
        b = torch.tensor([boxes], dtype=torch.float32, device=DEV)
        s = torch.tensor([scores], dtype=torch.float32, device=DEV)
        cl = None if classes is None else torch.tensor([classes], dtype=torch.int32, device=DEV)
        keep, counts = DO.nms(b, s, thr, len(boxes), classes=cl)
        want_k, want_c = DC.host_nms(host, np.asarray([boxes], F32), np.asarray([scores], F32),
                                     None if classes is None else np.asarray([classes], np.int32), None, thr, len(boxes))
        assert np.array_equal(_np(keep), want_k) and np.array_equal(_np(counts), want_c)
        return _np(keep)[0, :int(counts[0])].tolist()

    pair = [[0, 0, 3, 1], [1, 0, 4, 1]]              # IoU exactly 0.5
    assert run(pair, [0.9, 0.8], 0.5) == [0, 1]
    assert run(pair, [0.9, 0.8], float(np.nextafter(F32(0.5), F32(0)))) == [0]
    assert run([[5, 5, 5, 5]] * 2, [0.9, 0.8], 0.0) == [0, 1]                   # NaN IoU suppresses nothing
    assert run([[10, 10, 50, 60]] * 3, [0.5, 0.7, 0.6], 0.45, classes=[0, 1, 0]) == [1, 2]
    far = [[100 * i, 0, 100 * i + 10, 10] for i in range(4)]
    assert run(far, [0.5, 0.75, 0.5, 0.75], 0.45) == [1, 3, 0, 2]               # equal scores: the index decides
    many = [[100 + 0.01 * i, 100, 200, 200] for i in range(1100)]               # all suppressed by the first
    assert run(many, list(np.linspace(0.9, 0.1, 1100)), 0.45) == [0]


@pytest.mark.parametrize("n,m", [(1, 1), (65, 3), (300, 1)])
def test_box_iou_bit_for_bit_the_host_build(host, DO, n, m):
    rng = np.random.default_rng(n * 7 + m)
    a, b = DC.make_boxes(rng, n, 2), DC.make_boxes(rng, m, 2)
    a[0] = b[0] = [5, 5, 5, 5]                       # 0 / 0: NaN on both sides
    got = DO.box_iou(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert tuple(got.shape) == (n, m)
    assert np.array_equal(_bits(got), _bits(DC.host_box_iou(host, a, b)))
    assert np.isnan(_np(got)[0, 0])


def test_special_scores_and_cut_by_hand(host, DO):
    conf = F32(0.7)
    scores = [conf, np.nextafter(conf, F32(1)), NAN, np.inf, 0.1, -np.inf]
    c = Case(len(scores), C=1, layout=0, box_format=1, conf=float(conf))
    pred = np.zeros((1, len(scores), 5), F32)
    for a in range(len(scores)):
        pred[0, a, :4] = [100 * a, 0, 100 * a + 10, 10]
    pred[0, :, 4] = np.asarray(scores, F32)
    dets, counts = DO.postprocess(torch.from_numpy(pred).to(DEV), _spec(DO, c))
    want_d, want_c = DC.host_postprocess(host, c, pred)
    assert _np(counts).tolist() == [[2, 2]] and np.array_equal(_bits(dets), _bits(want_d))
    assert _np(dets)[0, :2, 0].tolist() == [300.0, 100.0]


def test_verdict_modes_by_hand(host, DO):
    dets = np.zeros((4, 3, 6), F32)
    dets[:, 0] = [0, 0, 3, 1, 0.9, 2]                # IoU exactly 0.5 with the gt of image 0: not a match
    dets[:, 1] = [50, 50, 60, 60, 0.8, 7]
    counts = np.asarray([[2, 2], [2, 2], [2, 2], [0, 0]], np.int32)
    gt = np.asarray([[1, 0, 4, 1], [NAN, 0, 4, 1], [0, 0, 3, 1], [1, 0, 4, 1]], F32)
    d, c, g = (torch.from_numpy(a).to(DEV) for a in (dets, counts, gt))
    assert _np(DO.verdict(d, c, g, 2, 7, True, 0.5)[0]).tolist() == [4, 2, 7, 4]
    assert _np(DO.verdict(d, c, g, 2, None, True, 0.5)[0]).tolist() == [4, 7, 7, 4]
    assert _np(DO.verdict(d, c, g, 2, 7, False, 0.5)[0]).tolist() == [5, 2, 7, 5]
    for args in ((2, 7, True), (2, None, True), (2, 7, False), (2, 2, False)):
        hb, hbest = DC.host_verdict(host, dets, counts, gt, *args, 0.5)
        bits, best = DO.verdict(d, c, g, *args, 0.5)
        assert np.array_equal(_np(bits), hb) and np.array_equal(_bits(best), _bits(hbest))


def test_success_fn_behind_a_torch_head(DO):
    """3 tiny renders -> DetectorInput(letterbox) -> a seeded conv head [B,4+C,A] -> verdict, against the oracle applied
    to the head's output copied to the host."""
    from gsplat_attack.detector_input import DetectorInput, letterbox_geometry
    from gsplat_attack.detector_output import DetectorOutput, make_success_fn
    C, H, W = 3, 40, 56
    conv = torch.nn.Conv2d(3, 4 + C, 8, stride=8)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=torch.Generator().manual_seed(5)) * 0.1)
        conv.bias.zero_()
    conv = conv.to(DEV)
    grid = torch.stack(torch.meshgrid(torch.arange(8.0), torch.arange(8.0), indexing="ij"), 0).to(DEV) * 8 + 4   # cell centres (y, x)

    def head(x):                                     # [B,3,64,64] -> [B,4+C,64]: xc yc w h in canvas pixels, class scores
        f = conv(x - 0.5)
        xy = grid.flip(0)[None] + 4 * torch.tanh(f[:, :2])
        wh = 16 + 12 * torch.sigmoid(f[:, 2:4])
        return torch.cat([xy, wh, torch.sigmoid(3 * f[:, 4:])], 1).flatten(2)

    images = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(11)).to(DEV)
    di = DetectorInput(letterbox=(64, 64))
    scale, _, _, top, left = letterbox_geometry(H, W, (64, 64))
    out = DetectorOutput(layout=1, has_obj=False, box_format=0, conf=0.55, iou=0.45, max_det=30).from_letterbox(scale, left, top)
    # in the render's frame: on a class-0 detection of view 0, none for view 1, on a class-2 detection of view 2
    gt = torch.tensor([[29.0, 8.0, 49.0, 26.0], [NAN] * 4, [30.0, 22.0, 48.0, 41.0]])
    with torch.no_grad():
        raw = head(di(images))
    assert tuple(raw.shape) == (3, 4 + C, 64)
    c = Case(64, C=C, B=3, layout=1, conf=0.55, iou=0.45, max_det=30,
             affine=(float(left), float(top), float(F32(1.0 / scale)), float(F32(1.0 / scale))))
    dets, counts, gap = DC.oracle_postprocess(c, _np(raw))
    assert gap > DC.MARGIN and counts[:, 0].min() > 0
    seen = set()
    for target, untarget, targeted in ((0, None, True), (1, 2, True), (2, 0, False)):
        bits, _, vgap = DC.oracle_verdict(dets, counts, gt.numpy(), target, untarget, targeted, 0.5)
        assert vgap > DC.MARGIN
        fn = make_success_fn(head, di, out, gt, target, untarget, targeted)
        flags = fn.batch_success(images)
        seen.add(tuple(flags))
        assert flags == [bool(b & 1) for b in bits]
        assert [fn(images[i], i) for i in range(3)] == [bool(b & 1) for b in bits]
    assert len(seen) > 1                             # the modes do not all give one answer
    got_d, got_c = out.detections(raw)
    assert np.array_equal(_np(got_c), counts) and np.array_equal(_bits(got_d), _bits(dets))

"""The detector output stage's C ABI and Python surface, the parts that need no GPU: symbols and argument counts, the
capability bit next to an unchanged version, every argument check (refused before any device call: the pointers handed
over are never followed), the workspace size's monotonicity, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import detect_ops as DO
from gsplat_attack import detector_output as DOUT

INVALID = 1
FAKE = 0x1000          # a non-null, 8-byte aligned pointer that is never followed: every call below is refused first
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    return DO._lib()


def _spec(**kw):
    v = dict(B=1, A=100, C=3, layout=1, has_obj=0, box_format=0, conf_thr=0.5, iou_thr=0.45, max_candidates=64, max_det=16,
             flags=0, ox=0.0, oy=0.0, sx=1.0, sy=1.0)
    v.update(kw)
    return DO._CDetSpec(*(v[k] for k, _ in DO._CDetSpec._fields_))


def _ws(lib, cs):
    n = ctypes.c_int64(-1)
    assert lib.gsr_det_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0
    return n.value


def test_symbols_version_and_capability(lib):
    assert len(lib.gsr_det_workspace_bytes.argtypes) == 2
    assert len(lib.gsr_det_postprocess.argtypes) == 7
    assert len(lib.gsr_det_nms.argtypes) == 13
    assert len(lib.gsr_det_box_iou.argtypes) == 6
    assert len(lib.gsr_det_verdict.argtypes) == 12
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(3, ctypes.byref(out)) == 0 and out.value & 2 and out.value & 1
    assert DO.available()
    # the struct of include/gsraster.h: fifteen 4-byte fields, no padding
    assert ctypes.sizeof(DO._CDetSpec) == 60 and DO._CDetSpec.conf_thr.offset == 24 and DO._CDetSpec.ox.offset == 44


BAD_SPECS = [dict(B=0), dict(A=0), dict(C=0), dict(B=-1), dict(layout=2), dict(layout=-1), dict(has_obj=2), dict(box_format=2),
             dict(max_candidates=0), dict(max_candidates=4097), dict(max_det=0), dict(max_det=65), dict(flags=2),
             dict(B=1 << 20, A=1 << 20), dict(B=1 << 10, A=1 << 16, C=80), dict(B=1 << 20, A=1, max_candidates=4096, max_det=4096)]


@pytest.mark.parametrize("bad", BAD_SPECS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_spec_checks(lib, bad):
    cs = _spec(**bad)
    n = ctypes.c_int64(-1)
    assert lib.gsr_det_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == INVALID and n.value == -1
    assert b"gsr_det_workspace_bytes:" in lib.gsr_last_error()
    assert lib.gsr_det_postprocess(ctypes.byref(cs), FAKE, FAKE, BIG, FAKE, FAKE, None) == INVALID
    assert b"gsr_det_postprocess:" in lib.gsr_last_error()


def test_postprocess_pointer_and_workspace_checks(lib):
    cs = _spec()
    need = _ws(lib, cs)
    assert need > 0
    for args in ((None, FAKE, FAKE, BIG, FAKE, FAKE), (ctypes.byref(cs), None, FAKE, BIG, FAKE, FAKE),
                 (ctypes.byref(cs), FAKE, None, BIG, FAKE, FAKE), (ctypes.byref(cs), FAKE, FAKE, BIG, None, FAKE),
                 (ctypes.byref(cs), FAKE, FAKE, BIG, FAKE, None)):
        assert lib.gsr_det_postprocess(*args, None) == INVALID
        assert b"gsr_det_postprocess:" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    assert lib.gsr_det_postprocess(ctypes.byref(cs), FAKE, FAKE, need - 1, FAKE, FAKE, None) == INVALID
    assert b"workspace" in lib.gsr_last_error()
    assert lib.gsr_det_postprocess(ctypes.byref(cs), FAKE, FAKE + 4, BIG, FAKE, FAKE, None) == INVALID
    assert b"aligned" in lib.gsr_last_error()
    assert lib.gsr_det_workspace_bytes(ctypes.byref(cs), None) == INVALID and b"null" in lib.gsr_last_error()


def test_workspace_bytes_is_monotone(lib):
    by_a = [_ws(lib, _spec(A=a)) for a in (1, 63, 64, 65, 1023, 8400, 25200)]
    assert by_a == sorted(by_a) and by_a[0] < by_a[-1]
    by_c = [_ws(lib, _spec(A=8400, max_candidates=m, max_det=1)) for m in (1, 64, 65, 1000, 4096)]
    assert by_c == sorted(by_c) and by_c[0] < by_c[-1]
    by_b = [_ws(lib, _spec(B=b)) for b in (1, 2, 8)]
    assert by_b == sorted(by_b) and by_b[0] < by_b[-1]
    # neither the class count nor max_det takes workspace
    assert _ws(lib, _spec(C=80)) == _ws(lib, _spec(C=1)) and _ws(lib, _spec(max_det=1)) == _ws(lib, _spec(max_det=64))


def test_nms_checks(lib):
    ok = dict(B=1, n=10, boxes=FAKE, scores=FAKE, classes=None, n_valid=None, iou=0.45, max_det=5, ws=FAKE, ws_bytes=BIG,
              keep=FAKE, counts=FAKE)
    need = _ws(lib, _spec(B=1, A=10, C=1, max_candidates=10, max_det=5))
    for bad in (dict(B=0), dict(n=0), dict(n=4097), dict(max_det=0), dict(max_det=11), dict(boxes=None), dict(scores=None),
                dict(ws=None), dict(keep=None), dict(counts=None), dict(ws_bytes=need - 1), dict(ws=FAKE + 4),
                dict(B=1 << 20, n=4096, max_det=1)):
        v = dict(ok)
        v.update(bad)
        assert lib.gsr_det_nms(v["B"], v["n"], v["boxes"], v["scores"], v["classes"], v["n_valid"], v["iou"], v["max_det"], v["ws"],
                               v["ws_bytes"], v["keep"], v["counts"], None) == INVALID, bad
        assert b"gsr_det_nms:" in lib.gsr_last_error()


def test_box_iou_and_verdict_checks(lib):
    for args in ((None, 1, FAKE, 1, FAKE), (FAKE, 1, None, 1, FAKE), (FAKE, 1, FAKE, 1, None), (FAKE, 0, FAKE, 1, FAKE),
                 (FAKE, 1, FAKE, -2, FAKE), (FAKE, 1 << 16, FAKE, 1 << 16, FAKE)):
        assert lib.gsr_det_box_iou(*args, None) == INVALID
        assert b"gsr_det_box_iou:" in lib.gsr_last_error()
    ok = dict(dets=FAKE, counts=FAKE, B=2, max_det=10, verdict=FAKE, best=FAKE)
    for bad in (dict(dets=None), dict(counts=None), dict(verdict=None), dict(best=None), dict(B=0), dict(max_det=0),
                dict(B=1 << 20, max_det=1 << 10)):
        v = dict(ok)
        v.update(bad)
        assert lib.gsr_det_verdict(v["dets"], v["counts"], v["B"], v["max_det"], None, 0, -1, 1, 0.5, v["verdict"], v["best"],
                                   None) == INVALID, bad
        assert b"gsr_det_verdict:" in lib.gsr_last_error()


def test_cpu_tensors_raise():
    raw = torch.zeros(1, 7, 20)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DO.postprocess(raw, DO.DetSpec())
    with pytest.raises(RuntimeError, match="no CPU path"):
        DO.nms(torch.zeros(1, 5, 4), torch.zeros(1, 5), 0.45, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DO.box_iou(torch.zeros(2, 4), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        DO.verdict(torch.zeros(1, 4, 6), torch.zeros(1, 2, dtype=torch.int32), None, 0)
    out = DOUT.DetectorOutput(layout=1, has_obj=False, box_format=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        out.detections(raw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        out.verdict(raw, None, 0)
    fn = DOUT.make_success_fn(lambda x: raw, None, out, None, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(torch.zeros(3, 8, 8), 0)
    with pytest.raises(ValueError, match="max_det"):
        DOUT.DetectorOutput(layout=1, has_obj=False, box_format=0, max_det=5000)
    with pytest.raises(ValueError, match="layout"):
        DOUT.DetectorOutput(layout=2, has_obj=False, box_format=0)


def test_affine_back_to_the_render_frame():
    base = DOUT.DetectorOutput(layout=1, has_obj=False, box_format=0, conf=0.25)
    assert (base.spec.ox, base.spec.oy, base.spec.sx, base.spec.sy) == (0.0, 0.0, 1.0, 1.0)
    lb = base.from_letterbox(1 / 3, 0, 140)          # a 1080p render letterboxed to 640 x 640
    assert (lb.spec.ox, lb.spec.oy) == (0.0, 140.0) and lb.spec.sx == lb.spec.sy == 1.0 / (1 / 3)
    assert lb.spec.conf_thr == 0.25 and base.spec.oy == 0.0      # a new object; the rest is carried over
    rs = base.from_resize((1080, 1920), (1088, 1920))            # predict_and_save's resize to a multiple of 32
    assert (rs.spec.ox, rs.spec.oy, rs.spec.sx, rs.spec.sy) == (0.0, 0.0, 1.0, 1080 / 1088)

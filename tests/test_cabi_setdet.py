"""The set-prediction detector stage's C ABI and Python surface, the parts that need no GPU: symbols, the capability bit
next to the unchanged bits and version, the struct layout, every argument check (refused before any device call: the
pointers handed over are never followed), the workspace size, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import setdet_ops as SO
from gsplat_attack import set_detector as SD

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    return SO._lib()


def _spec(B=2, Q=8, C=3, M=2, **kw):
    cs = SO.c_spec(SO.SetDetSpec(img_w=640.0, img_h=480.0), B, Q, C, M)
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


def _ws(lib, cs):
    n = ctypes.c_int64(-1)
    assert lib.gsr_setdet_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0, lib.gsr_last_error()
    return n.value


def _loss(lib, cs, logits=FAKE, boxes=FAKE, gtb=FAKE, gtc=FAKE, ws=FAKE, ws_bytes=BIG, loss=FAKE, gl=FAKE, gb=FAKE, match=None,
          tgt=None):
    return lib.gsr_setdet_loss(ctypes.byref(cs) if cs is not None else None, logits, boxes, gtb, gtc, ws, ws_bytes, loss, gl, gb,
                               match, tgt, None)


def _post(lib, cs, logits=FAKE, boxes=FAKE, dets=FAKE, counts=FAKE):
    return lib.gsr_setdet_postprocess(ctypes.byref(cs) if cs is not None else None, logits, boxes, dets, counts, None)


def test_symbols_version_and_capability(lib):
    assert len(lib.gsr_setdet_workspace_bytes.argtypes) == 2
    assert len(lib.gsr_setdet_loss.argtypes) == 13
    assert len(lib.gsr_setdet_postprocess.argtypes) == 6
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(3, ctypes.byref(out)) == 0 and out.value == 1 | 2 | 4 | 8
    assert SO.available() and SO.GSR_CAP_SETDET == 8
    # the struct of include/gsraster.h: sixteen 4-byte fields in the stated order, no padding
    names = ["B", "Q", "C", "M", "img_w", "img_h", "c_class", "c_l1", "c_giou", "w_ce", "w_l1", "w_giou", "eos_coef", "conf_thr",
             "max_det", "flags"]
    assert [f[0] for f in SO._CSetDetSpec._fields_] == names and ctypes.sizeof(SO._CSetDetSpec) == 64
    assert [getattr(SO._CSetDetSpec, n).offset for n in names] == list(range(0, 64, 4))
    d = SO.SetDetSpec()
    assert (d.c_class, d.c_l1, d.c_giou, d.w_ce, d.w_l1, d.w_giou, d.eos_coef, d.conf_thr) == (1, 5, 2, 1, 5, 2, 0.1, 0.7)


NAN, INF = float("nan"), float("inf")
BAD_SPECS = [dict(B=0), dict(B=-1), dict(B=65536), dict(Q=0), dict(Q=1025), dict(C=0), dict(C=1025), dict(M=0), dict(M=33, Q=64),
             dict(Q=1, M=2), dict(Q=5, M=6), dict(max_det=0), dict(max_det=1025), dict(flags=1), dict(flags=0x80000000),
             dict(c_class=-1.0), dict(c_l1=NAN), dict(c_giou=INF), dict(w_ce=-0.5), dict(w_l1=INF), dict(w_giou=NAN),
             dict(eos_coef=-0.1), dict(eos_coef=NAN), dict(img_w=0.0), dict(img_w=-640.0), dict(img_h=NAN), dict(img_h=INF),
             dict(B=4096, Q=1024, C=1024)]


@pytest.mark.parametrize("bad", BAD_SPECS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_spec_checks(lib, bad):
    cs = _spec(**bad)
    n = ctypes.c_int64(-1)
    assert lib.gsr_setdet_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == INVALID and n.value == -1
    assert b"gsr_setdet_workspace_bytes:" in lib.gsr_last_error()
    assert _loss(lib, cs) == INVALID
    assert b"gsr_setdet_loss:" in lib.gsr_last_error()
    assert _post(lib, cs) == INVALID
    assert b"gsr_setdet_postprocess:" in lib.gsr_last_error()


def test_the_limits_themselves_are_accepted(lib):
    for ok in (dict(B=65535, Q=1, C=1, M=1), dict(B=1, Q=1024, C=1024, M=32), dict(Q=2, M=2), dict(eos_coef=0.0),
               dict(w_ce=0.0, w_l1=0.0, w_giou=0.0), dict(max_det=1), dict(max_det=1024)):
        assert _ws(lib, _spec(**ok)) > 0, ok
    cs = _spec(Q=5, M=6)
    assert _loss(lib, cs) == INVALID and b"Q >= M" in lib.gsr_last_error()


def test_pointer_and_workspace_checks(lib):
    cs = _spec()
    need = _ws(lib, cs)
    assert need > 0
    for bad in (dict(logits=None), dict(boxes=None), dict(gtb=None), dict(gtc=None), dict(ws=None), dict(loss=None)):
        assert _loss(lib, cs, **bad) == INVALID, bad
        assert b"gsr_setdet_loss:" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    assert _loss(lib, None) == INVALID and b"null spec" in lib.gsr_last_error()
    assert _loss(lib, cs, ws_bytes=need - 1) == INVALID and b"workspace" in lib.gsr_last_error()
    assert _loss(lib, cs, ws=FAKE + 8) == INVALID and b"aligned" in lib.gsr_last_error()
    assert _loss(lib, cs, logits=FAKE + 2) == INVALID and b"aligned" in lib.gsr_last_error()
    assert _loss(lib, cs, match=FAKE + 1) == INVALID and b"aligned" in lib.gsr_last_error()
    assert lib.gsr_setdet_workspace_bytes(ctypes.byref(cs), None) == INVALID and b"null" in lib.gsr_last_error()
    for bad in (dict(logits=None), dict(boxes=None), dict(dets=None), dict(counts=None)):
        assert _post(lib, cs, **bad) == INVALID, bad
        assert b"gsr_setdet_postprocess:" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    assert _post(lib, None) == INVALID and b"null spec" in lib.gsr_last_error()
    assert _post(lib, cs, dets=FAKE + 2) == INVALID and b"aligned" in lib.gsr_last_error()


def test_workspace_bytes_is_monotone(lib):
    for key, vals in (("B", (1, 2, 64)), ("Q", (32, 100, 900)), ("M", (1, 8, 32)), ("C", (1, 91, 1024))):
        got = [_ws(lib, _spec(**{"Q": 64, key: v})) for v in vals]
        assert got == sorted(got) and got[0] < got[-1], key
    # DETR's own shape: the statistics, one [B,M,Q] cost matrix, tgt and the slab -- well under a megabyte
    full = _spec(B=8, Q=100, C=91, M=1)
    assert 8 * 100 * 4 * 4 <= _ws(lib, full) < 1 << 20


def test_cpu_tensors_raise():
    logits, boxes = torch.zeros(1, 8, 4), torch.zeros(1, 8, 4)
    gtb, gtc = torch.zeros(1, 1, 4), torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SO.run(logits, boxes, gtb, gtc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SO.setdet_loss(logits, boxes, gtb, gtc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SO.postprocess(logits, boxes)
    sl = SD.SetDetectorLoss(3, (640, 480))
    with pytest.raises(RuntimeError, match="no CPU path"):
        sl.loss(logits, boxes, gtb, gtc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sl.matching(logits, boxes, gtb, gtc)
    so = SD.SetDetectorOutput((640, 480))
    with pytest.raises(RuntimeError, match="no CPU path"):
        so.detect(logits, boxes)
    with pytest.raises(RuntimeError, match="no CPU path"):
        so.verdicts(logits, boxes, torch.zeros(1, 4), 0)
    fn = SD.make_set_loss_fn(lambda x: {"pred_logits": logits, "pred_boxes": boxes}, None, sl, torch.zeros(2, 4), 0)
    assert fn.takes_view_index is True
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(torch.zeros(1, 3, 64, 64), idx=[1])
    with pytest.raises(ValueError, match="view indices"):
        fn(torch.zeros(2, 3, 64, 64), idx=[1])


def test_python_argument_checks():
    import gsplat_attack
    assert gsplat_attack.SetDetectorLoss is SD.SetDetectorLoss and gsplat_attack.SetDetectorOutput is SD.SetDetectorOutput
    assert gsplat_attack.make_set_loss_fn is SD.make_set_loss_fn
    with pytest.raises(ValueError, match="nc"):
        SD.SetDetectorLoss(0, (640, 480))
    with pytest.raises(ValueError, match="weights"):
        SD.SetDetectorLoss(3, (640, 480), giou=-1.0)
    with pytest.raises(ValueError, match="frame"):
        SD.SetDetectorLoss(3, (0, 480))
    with pytest.raises(ValueError, match="max_det"):
        SD.SetDetectorOutput((640, 480), max_det=0)
    sl = SD.SetDetectorLoss(3, (640, 480), l1=4.0, eos_coef=0.2)
    assert (sl.spec.img_w, sl.spec.img_h, sl.spec.w_l1, sl.spec.eos_coef, sl.spec.c_l1) == (640.0, 480.0, 4.0, 0.2, 5.0)
    with pytest.raises(ValueError, match="logits"):
        sl.loss(torch.zeros(1, 8, 5), torch.zeros(1, 8, 4), torch.zeros(1, 1, 4), torch.zeros(1, 1))
    gb, gc = sl._gt(torch.tensor([[300.0, 100.0, 400.0, 300.0], [float("nan")] * 4]), torch.tensor([2, 2]), "cpu")
    assert gb.shape == (2, 1, 4) and gc.tolist() == [[2], [-1]]                   # a NaN box: the row is absent

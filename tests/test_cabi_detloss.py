"""The detector loss stage's C ABI and Python surface, the parts that need no GPU: symbols, the capability bit next to an
unchanged version, every argument check (refused before any device call: the pointers handed over are never followed),
the workspace size, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import detloss_ops as LO
from gsplat_attack import detector_loss as DL

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
BIG = 1 << 40
LEVELS = [(8, 8, 8.0), (4, 4, 16.0), (2, 2, 32.0)]


@pytest.fixture(scope="module")
def lib():
    return LO._lib()


def _spec(levels=LEVELS, B=2, C=3, M=2, **kw):
    cs = LO.c_spec(LO.DetLossSpec(), levels, B, C, M)
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


def _ws(lib, cs):
    n = ctypes.c_int64(-1)
    assert lib.gsr_detloss_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0, lib.gsr_last_error()
    return n.value


def _call(lib, cs, pred=FAKE, gtb=FAKE, gtc=FAKE, ws=FAKE, ws_bytes=BIG, loss=FAKE, grad=FAKE, tgt=None, ts=None):
    return lib.gsr_detloss(ctypes.byref(cs) if cs is not None else None, pred, gtb, gtc, ws, ws_bytes, loss, grad, tgt, ts, None)


def test_symbols_version_and_capability(lib):
    assert len(lib.gsr_detloss_workspace_bytes.argtypes) == 2
    assert len(lib.gsr_detloss.argtypes) == 11
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(3, ctypes.byref(out)) == 0 and out.value & 4 and out.value & 2 and out.value & 1
    assert LO.available() and LO.GSR_CAP_DETLOSS == 4
    # the struct of include/gsraster.h: twenty-eight 4-byte fields, no padding
    assert ctypes.sizeof(LO._CDetLossSpec) == 112 and LO._CDetLossSpec.level_stride.offset == 60
    assert LO._CDetLossSpec.reg_max.offset == 80 and LO._CDetLossSpec.flags.offset == 108


BAD_SPECS = [dict(B=0), dict(A=0), dict(C=0), dict(B=-1), dict(M=0), dict(M=33), dict(nl=0), dict(nl=6), dict(reg_max=8),
             dict(reg_max=17), dict(topk=0), dict(topk=17), dict(flags=1), dict(alpha=-1.0), dict(beta=float("nan")),
             dict(w_box=float("inf")), dict(w_cls=-0.5), dict(w_dfl=float("nan")), dict(A=85), dict(A=83), dict(B=65536),
             dict(B=1 << 14, A=1 << 20)]


@pytest.mark.parametrize("bad", BAD_SPECS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_spec_checks(lib, bad):
    cs = _spec(**bad)
    n = ctypes.c_int64(-1)
    assert lib.gsr_detloss_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == INVALID and n.value == -1
    assert b"gsr_detloss_workspace_bytes:" in lib.gsr_last_error()
    assert _call(lib, cs) == INVALID
    assert b"gsr_detloss:" in lib.gsr_last_error()


def test_level_checks(lib):
    for levels in ([(0, 8, 8.0)], [(8, -1, 8.0)], [(8, 8, 0.0)], [(8, 8, -8.0)], [(8, 8, float("nan"))], [(8, 8, float("inf"))],
                   [(1 << 16, 1 << 16, 8.0)]):
        cs = _spec(levels=levels)
        assert _call(lib, cs) == INVALID, levels
        assert b"gsr_detloss:" in lib.gsr_last_error()
    # the levels must add up to A: the message names both numbers
    cs = _spec(A=85)
    assert _call(lib, cs) == INVALID and b"84" in lib.gsr_last_error() and b"85" in lib.gsr_last_error()


def test_pointer_and_workspace_checks(lib):
    cs = _spec()
    need = _ws(lib, cs)
    assert need > 0
    for bad in (dict(pred=None), dict(gtb=None), dict(gtc=None), dict(ws=None), dict(loss=None)):
        assert _call(lib, cs, **bad) == INVALID, bad
        assert b"gsr_detloss:" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    assert _call(lib, None) == INVALID and b"null spec" in lib.gsr_last_error()
    assert _call(lib, cs, ws_bytes=need - 1) == INVALID and b"workspace" in lib.gsr_last_error()
    assert _call(lib, cs, ws=FAKE + 8) == INVALID and b"aligned" in lib.gsr_last_error()
    assert _call(lib, cs, pred=FAKE + 2) == INVALID and b"aligned" in lib.gsr_last_error()
    assert _call(lib, cs, tgt=FAKE + 1) == INVALID and b"aligned" in lib.gsr_last_error()
    assert lib.gsr_detloss_workspace_bytes(ctypes.byref(cs), None) == INVALID and b"null" in lib.gsr_last_error()


def test_workspace_bytes_is_monotone(lib):
    by_b = [_ws(lib, _spec(B=b)) for b in (1, 2, 8)]
    assert by_b == sorted(by_b) and by_b[0] < by_b[-1]
    by_m = [_ws(lib, _spec(M=m)) for m in (1, 2, 32)]
    assert by_m == sorted(by_m) and by_m[0] < by_m[-1]
    by_a = [_ws(lib, _spec(levels=[(n, n, 8.0)])) for n in (1, 8, 80, 200)]
    assert by_a == sorted(by_a) and by_a[0] < by_a[-1]
    # the reference's shape: two [B,M,A] arrays, two [B,A] arrays and the slab -- well under a megabyte
    full = _spec(levels=[(80, 80, 8.0), (40, 40, 16.0), (20, 20, 32.0)], B=2, C=80, M=1)
    assert 4 * 2 * 8400 * 4 <= _ws(lib, full) < 1 << 20


def test_cpu_tensors_raise():
    pred = torch.zeros(1, 64 + 3, 84)
    gtb, gtc = torch.zeros(1, 1, 4), torch.zeros(1, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LO.run(pred, LEVELS, gtb, gtc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LO.detloss(pred, LEVELS, gtb, gtc)
    dl = DL.DetectorLoss(3, input_hw=(64, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dl.loss(pred, gtb, gtc)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dl.assignment([torch.zeros(1, 67, 8, 8), torch.zeros(1, 67, 4, 4), torch.zeros(1, 67, 2, 2)], gtb, gtc)
    fn = DL.make_loss_fn(lambda x: pred, None, dl, torch.zeros(2, 4), 0)
    assert fn.takes_view_index is True
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(torch.zeros(1, 3, 64, 64), idx=[1])
    with pytest.raises(ValueError, match="view indices"):
        fn(torch.zeros(2, 3, 64, 64), idx=[1])


def test_python_argument_checks():
    with pytest.raises(ValueError, match="nc"):
        DL.DetectorLoss(0)
    with pytest.raises(ValueError, match="topk"):
        DL.DetectorLoss(3, topk=17)
    with pytest.raises(ValueError, match="strides"):
        DL.DetectorLoss(3, strides=(1, 2, 4, 8, 16, 32))
    dl = DL.DetectorLoss(3)
    with pytest.raises(ValueError, match="input_hw"):
        dl.loss(torch.zeros(1, 67, 84), torch.zeros(1, 1, 4), torch.zeros(1, 1))
    with pytest.raises(ValueError, match="channels"):
        dl.loss([torch.zeros(1, 66, 8, 8), torch.zeros(1, 66, 4, 4), torch.zeros(1, 66, 2, 2)], torch.zeros(1, 1, 4), torch.zeros(1, 1))
    with pytest.raises(ValueError, match="feature maps"):
        dl.loss([torch.zeros(1, 67, 8, 8)], torch.zeros(1, 1, 4), torch.zeros(1, 1))


def test_to_letterbox_maps_render_frame_boxes():
    base = DL.DetectorLoss(80)
    assert base.affine == (1.0, 0.0, 0.0)
    lb = base.to_letterbox(1 / 3, 0, 140)          # a 1080p render letterboxed to 640 x 640
    assert lb.affine == (1 / 3, 0.0, 140.0) and base.affine == (1.0, 0.0, 0.0) and lb.spec == base.spec
    gb, gc = lb._gt(torch.tensor([[300.0, 600.0, 900.0, 900.0], [float("nan")] * 4]), torch.tensor([7, 7]), "cpu")
    assert gb.shape == (2, 1, 4) and gc.tolist() == [[7], [-1]]                   # a NaN box: the row is absent
    assert torch.allclose(gb[0, 0], torch.tensor([100.0, 340.0, 300.0, 440.0]))  # x * scale + pad_left, y * scale + pad_top

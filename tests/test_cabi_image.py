"""The image front end's C ABI and Python surface, the parts that need no GPU: symbols and argument counts, the
capability bit, every argument check (refused before any device call), CPU tensors (no fallback), and the detector-input
geometry against the reference wrappers' formula."""
import ctypes

import pytest
import torch

import diff_gaussian_rasterization as D
from diff_gaussian_rasterization import image_ops as IO
from gsplat_attack import detector_input as DI

INVALID = 1
FAKE = 0x1000          # a non-null pointer that is never followed: every call below is refused first


@pytest.fixture(scope="module")
def lib():
    return IO._lib()


def test_symbols_version_and_capability(lib):
    assert len(lib.gsr_image_resample.argtypes) == 4
    assert len(lib.gsr_image_resample_backward.argtypes) == 6
    assert len(lib.gsr_image_to_u8.argtypes) == 6
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(3, ctypes.byref(out)) == 0 and out.value & 1
    assert IO.available()
    # the struct of include/gsraster.h: ten int32, a float, (padding,) two pointers, a uint32
    assert IO._CResample.mean.offset == 48 and IO._CResample.flags.offset == 64 and ctypes.sizeof(IO._CResample) == 72


def _spec(**kw):
    v = dict(B=1, C=3, H=8, W=8, out_h=4, out_w=4, rh=4, rw=4, top=0, left=0)
    v.update(kw)
    return IO._CResample(v["B"], v["C"], v["H"], v["W"], v["out_h"], v["out_w"], v["rh"], v["rw"], v["top"], v["left"], 0.0,
                         None, None, v.get("flags", 0))


BAD_SPECS = [dict(B=0), dict(C=0), dict(C=5), dict(H=0), dict(W=-1), dict(out_h=0), dict(out_w=0), dict(rh=0), dict(rw=0),
             dict(top=-1), dict(left=-1), dict(top=1), dict(left=1), dict(rh=5, out_h=4), dict(top=2 ** 31 - 1),
             dict(H=65536, W=65536), dict(B=1024, H=1024, W=1024, C=3), dict(out_h=65536, out_w=65536, rh=1, rw=1),
             dict(flags=2)]


@pytest.mark.parametrize("bad", BAD_SPECS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_spec_checks(lib, bad):
    cs = _spec(**bad)
    assert lib.gsr_image_resample(ctypes.byref(cs), FAKE, FAKE, None) == INVALID
    assert b"gsr_image_resample:" in lib.gsr_last_error()
    assert lib.gsr_image_resample_backward(ctypes.byref(cs), FAKE, FAKE, FAKE, 0, None) == INVALID
    assert b"gsr_image_resample_backward:" in lib.gsr_last_error()


def test_null_pointer_checks(lib):
    cs = _spec()
    for args in ((None, FAKE, FAKE), (ctypes.byref(cs), None, FAKE), (ctypes.byref(cs), FAKE, None)):
        assert lib.gsr_image_resample(*args, None) == INVALID
        assert b"gsr_image_resample:" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    for args in ((None, FAKE, FAKE, FAKE), (ctypes.byref(cs), None, None, FAKE), (ctypes.byref(cs), None, FAKE, None)):
        assert lib.gsr_image_resample_backward(*args, 0, None) == INVALID
        assert b"gsr_image_resample_backward:" in lib.gsr_last_error() and b"null" in lib.gsr_last_error()
    clamp = _spec(flags=1)                       # the clamp's mask needs the source
    assert lib.gsr_image_resample_backward(ctypes.byref(clamp), None, FAKE, FAKE, 0, None) == INVALID
    assert b"gsr_image_resample_backward:" in lib.gsr_last_error() and b"src" in lib.gsr_last_error()
    for args in ((None, 1, 4, 4, FAKE), (FAKE, 1, 4, 4, None), (FAKE, 0, 4, 4, FAKE), (FAKE, 1, 0, 4, FAKE), (FAKE, 1, 4, -3, FAKE),
                 (FAKE, 1, 65536, 65536, FAKE), (FAKE, 1024, 1024, 1024, FAKE)):
        assert lib.gsr_image_to_u8(*args, None) == INVALID
        assert b"gsr_image_to_u8:" in lib.gsr_last_error()


def test_cpu_tensors_raise():
    x = torch.zeros(1, 3, 8, 8)
    spec = IO.ResampleSpec(4, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        IO.resample(x, spec)
    with pytest.raises(RuntimeError, match="no CPU path"):
        IO.resample_backward(torch.zeros(1, 3, 4, 4), spec, x.shape)
    with pytest.raises(RuntimeError, match="no CPU path"):
        IO.to_uint8_hwc(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DI.letterbox(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DI.resize_shorter_side(x, 16, mean=(0.5, 0.5, 0.5), std=(0.2, 0.2, 0.2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        DI.resize_to_multiple(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DI.with_detector_input(lambda t: t.sum(), DI.DetectorInput(letterbox=(16, 16)))(x)
    with pytest.raises(ValueError, match="exactly one"):
        DI.DetectorInput()
    with pytest.raises(ValueError, match="exactly one"):
        DI.DetectorInput(letterbox=(8, 8), multiple=32)


@pytest.mark.parametrize("H,W", [(1080, 1920), (900, 1601), (481, 640), (640, 640), (2160, 3840)])
@pytest.mark.parametrize("new_shape", [(640, 640), (384, 640)])
def test_letterbox_geometry(H, W, new_shape):
    # the wrappers' formula, written out
    new_h, new_w = new_shape
    scale = min(new_h / H, new_w / W)
    resized_h, resized_w = int(round(H * scale)), int(round(W * scale))
    pad_top, pad_left = (new_h - resized_h) // 2, (new_w - resized_w) // 2
    assert DI.letterbox_geometry(H, W, new_shape) == (scale, resized_h, resized_w, pad_top, pad_left)
    assert resized_h <= new_h and resized_w <= new_w and (resized_h == new_h or resized_w == new_w)


def test_letterbox_geometry_literals():
    assert DI.letterbox_geometry(1080, 1920) == (1 / 3, 360, 640, 140, 0)
    assert DI.letterbox_geometry(900, 1601)[1:] == (360, 640, 140, 0)
    assert DI.letterbox_geometry(481, 640) == (1.0, 481, 640, 79, 0)
    assert DI.letterbox_geometry(640, 640) == (1.0, 640, 640, 0, 0)
    assert DI.letterbox_geometry(2160, 3840)[1:] == (360, 640, 140, 0)


def test_letterbox_boxes_literals():
    # (x1, y1, x2, y2) = (100, 200, 500, 800) px of a 1080p render, letterboxed to 640 x 640: scale 1/3, 140 rows of pad on top
    box = torch.tensor([[[100.0, 200.0, 500.0, 800.0]]], dtype=torch.float64)
    got = DI.letterbox_boxes(box, 1 / 3, 0, 140, (640, 640))
    want = torch.tensor([[[0.15625, 0.4791666666666667, 0.20833333333333334, 0.3125]]], dtype=torch.float64)
    assert got.shape == (1, 1, 4) and torch.allclose(got, want, rtol=0, atol=1e-15)
    # a non-square canvas and a left pad: x over the width, y over the height
    got = DI.letterbox_boxes(torch.tensor([0.0, 0.0, 100.0, 50.0], dtype=torch.float64), 2.0, 20, 6, (128, 256))
    assert torch.allclose(got, torch.tensor([120 / 256, 56 / 128, 200 / 256, 100 / 128], dtype=torch.float64), rtol=0, atol=1e-15)


def test_resize_sizes():
    assert DI.shorter_side_size(1080, 1920, 800) == (800, 1422)
    assert DI.shorter_side_size(1920, 1080, 800) == (1422, 800)
    assert DI.shorter_side_size(480, 640, 800) == (800, 1066)
    assert DI.shorter_side_size(800, 800, 800) == (800, 800)

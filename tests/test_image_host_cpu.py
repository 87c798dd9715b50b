"""csrc/gsr_image.h -- the scalar source the image front end's kernels compile -- built for the HOST
(tests/host_math/image_host.cpp) and compared with torch.nn.functional.interpolate in float64 and its autograd, within the
bounds derived in tests/image_cases.py.  No GPU, no product library involved."""
import os
import subprocess

import numpy as np
import pytest
import torch

import image_cases as IC
from image_cases import Case


@pytest.fixture(scope="module")
def lib():
    return IC.host_lib()


def _check(lib, c: Case):
    src, g = IC.make_inputs(c)
    out = IC.host_forward(lib, c, src)
    ref, gref, fb, bb = IC.oracle(c, src, g if c.backward else None)
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"{c.id}: forward err {err:.3e} bound {fb:.3e}")
    assert np.isfinite(out).all() and err <= fb, (c.id, err, fb)
    if not c.backward:
        return out, None
    grad, n_max = IC.host_backward(lib, c, src, g)
    gerr = float(np.abs(grad.astype(np.float64) - gref).max())
    print(f"{c.id}: backward err {gerr:.3e} bound {bb(n_max):.3e} n_max {n_max}")
    assert np.isfinite(grad).all() and gerr <= bb(n_max), (c.id, gerr, bb(n_max), n_max)
    return out, grad


@pytest.mark.parametrize("c", IC.RESIZES, ids=lambda c: c.id)
def test_resize_against_interpolate(lib, c):
    out, _ = _check(lib, c)
    if (c.H, c.W, c.rh, c.rw) == (1080, 1920, 360, 640):
        # scale 3 exactly: every sample sits on source pixel 3 d + 1 with weight 1
        src, _ = IC.make_inputs(c)
        assert np.array_equal(out, src[:, :, 1::3, 1::3])
    if (c.H, c.W) == (c.rh, c.rw):
        src, _ = IC.make_inputs(c)
        assert np.array_equal(out, src)                   # the identity


@pytest.mark.parametrize("c", IC.COMPOSED, ids=lambda c: c.id)
def test_pad_channels_clamp_normalise(lib, c):
    out, grad = _check(lib, c)
    src, _ = IC.make_inputs(c)
    inside = np.zeros((c.oh, c.ow), bool)
    inside[c.top:c.top + c.rh, c.left:c.left + c.rw] = True
    assert np.all(out[:, :, ~inside] == np.float32(c.pad))       # the pad as given, not normalised
    if c.clamp:
        # torch.clamp's inclusive mask: no gradient outside [0,1], gradient AT 0 and 1 (and -0.0)
        outside = (src < 0) | (src > 1)
        assert outside.any() and (src == 0).any() and (src == 1).any()
        assert np.all(grad[outside] == 0)


def test_terms_per_source_pixel(lib):
    c = Case(9, 16, 23, 37)
    src, g = IC.make_inputs(c)
    assert IC.host_backward(lib, c, src, g)[1] == 36


@pytest.mark.parametrize("c", [IC.RESIZES[4], IC.COMPOSED[0], IC.COMPOSED[2]], ids=lambda c: c.id)
def test_accumulate(lib, c):
    src, g = IC.make_inputs(c)
    grad, _ = IC.host_backward(lib, c, src, g)
    base = np.random.default_rng(5).standard_normal(grad.shape).astype(np.float32)
    acc, _ = IC.host_backward(lib, c, src, g, into=base)
    assert np.array_equal(acc, base + grad)                      # one float32 addition onto what was there


def test_every_source_pixel_written(lib):
    # a strong downscale: most source pixels are sampled by nothing and must come out as zero, not as what was there
    c = Case(37, 53, 2, 3)
    src, g = IC.make_inputs(c)
    grad, _ = IC.host_backward(lib, c, src, g)
    assert np.isfinite(grad).all() and (grad == 0).sum() > grad.size // 2
    _, gref, _, bb = IC.oracle(c, src, g)
    assert np.array_equal(grad == 0, gref == 0)


@pytest.mark.parametrize("n_in,n_out", [(1920, 640), (1920, 1422), (3840, 641), (7, 9), (16, 37), (53, 9), (1, 4), (3, 1),
                                        (64, 64), (1080, 1088), (65520, 800), (800, 65520)])
def test_inverse_range_is_exact(lib, n_in, n_out):
    """axis_range(s) = exactly the output indices whose forward taps name s, for every source index."""
    i01 = np.zeros(2, np.int32)
    l01 = np.zeros(2, np.float32)
    taps = np.zeros((n_out, 2), np.int64)
    for d in range(n_out):
        lib.ih_axis_sample(n_in, n_out, d, i01.ctypes.data, l01.ctypes.data)
        taps[d] = i01
        assert 0 <= i01[0] <= i01[1] <= n_in - 1 and i01[1] - i01[0] <= 1
        assert 0.0 <= l01[1] <= 1.0 and l01[0] == np.float32(1.0) - l01[1]
    lohi = np.zeros(2, np.int32)
    first = np.full(n_in, n_out, np.int64)
    last = np.full(n_in, -1, np.int64)
    for d in range(n_out):
        for s in set(taps[d]):
            first[s] = min(first[s], d)
            last[s] = max(last[s], d)
    for s in range(n_in):
        lib.ih_axis_range(n_in, n_out, s, lohi.ctypes.data)
        if last[s] < 0:
            assert lohi[0] > lohi[1], (s, lohi)
        else:
            assert (lohi[0], lohi[1]) == (first[s], last[s]), (s, lohi, first[s], last[s])


def test_to_u8_matches_torch(lib):
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                           np.array([0.0, 1.0, -0.0, -0.2, 1.2, 0.5], np.float32),
                           np.random.default_rng(0).uniform(-0.2, 1.2, 3 * 5 * 7 * 9 - 774).astype(np.float32)]).astype(np.float32)
    x = np.ascontiguousarray(vals.reshape(5, 3, 7, 9))
    out = np.zeros((5, 7, 9, 3), np.uint8)
    lib.ih_to_u8(x.ctypes.data, 5, 7, 9, out.ctypes.data)
    ref = (torch.from_numpy(x).clamp(0, 1) * 255).byte().permute(0, 2, 3, 1).contiguous().numpy()
    assert np.array_equal(out, ref)
    nan = np.full((1, 3, 1, 1), np.nan, np.float32)
    o1 = np.full((1, 1, 1, 3), 9, np.uint8)
    lib.ih_to_u8(nan.ctypes.data, 1, 1, 1, o1.ctypes.data)
    assert np.all(o1 == 0)


def test_sanitized_harness(tmp_path):
    """tests/host_math/image_harness.cpp: its own main over the three smallest shapes (plain and padded, C = 1 and 4,
    clamp and affine), built with AddressSanitizer and UBSan and run as a program."""
    exe = str(tmp_path / "image_harness")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", IC.CSRC, os.path.join(IC.HM, "image_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("image_harness ok"), r.stdout + r.stderr

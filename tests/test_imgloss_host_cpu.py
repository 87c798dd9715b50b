"""The fused image losses' scalar source on the host (tests/host_math/imgloss_host.cpp over csrc/gsr_imgloss.h) against the
oracle of tests/imgloss_cases.py, and that oracle against the reference's own outputs (tests/golden/ref_imgloss.npz) and
against float64 finite differences.  Needs no GPU."""
import os

import numpy as np
import pytest
import torch

import imgloss_cases as IC

CASES = IC.cases()
BY_NAME = {c.name: c for c in CASES}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_imgloss.npz")


def test_header_tile_and_taps_are_the_references():
    th, tw, taps = IC.header()
    assert th >= 1 and tw >= 1 and len(IC.shapes()) == 6 and IC.shapes()[3] == IC.GOLDEN_SHAPE
    assert np.array_equal(taps, IC.reference_taps()) and taps.dtype == np.float32
    with np.load(GOLDEN) as g:
        assert np.array_equal(taps, g["taps"])                      # what the reference's gaussian(11, 1.5) held
    from diff_gaussian_rasterization import imgloss_ops as IL
    assert IL.TILE == (th, tw)


def test_oracle_reproduces_the_reference_outputs():
    """The float64 oracle (separable window of the float32 taps) against the reference's float32 CPU run: within the 2^-22
    floor of every output (the 2-D window's one rounding per weight included)."""
    case = BY_NAME["x".join(map(str, IC.GOLDEN_SHAPE))]
    x, y = IC.inputs(case)
    with np.load(GOLDEN) as g:
        assert np.array_equal(g["img"], x) and np.array_equal(g["ref"], y)
        want = {k: g[k] for k in ("l1", "l2", "ssim_mean", "ssim_per_image", "psnr")}
    t = IC.run_arrays(x, y, (0.0, 0.0, 1.0), torch.float64)["terms"]
    got = dict(l1=t[:, 0].mean(), l2=t[:, 1].mean(), ssim_mean=t[:, 2].mean(), ssim_per_image=t[:, 2],
               psnr=(20 * torch.log10(1.0 / torch.sqrt(t[:, 1]))).view(-1, 1))
    for k, w in want.items():
        e = IC.err(torch.as_tensor(w), got[k])
        print(f"fixture {k}: err {e:.3e} floor {IC.FLOOR:.3e}")
        assert tuple(np.shape(w)) == tuple(got[k].shape) and e <= IC.FLOOR, (k, e)


@pytest.mark.parametrize("w", IC.WEIGHTS, ids=lambda w: "w" + "-".join(f"{v:g}" for v in w))
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_host_matches_the_oracle(c, w):
    assert IC.margins_ok(c)
    fails = IC.check(IC.host_run(c, w), IC.reference(c, w), f"host {c.id} {w}")
    assert not fails, fails


@pytest.mark.parametrize("name", ("1x1x1x1", "1x1x7x5"))
@pytest.mark.parametrize("w", ((0.8, 0.0, 0.2), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)))
def test_oracle_gradient_against_finite_differences(name, w):
    """Central differences in float64, h = 1e-6: truncation h^2 f''' / 6 and rounding 1e-16 / h are both below 1e-9 of the
    gradient's size here; held to 1e-6.  (A copied pixel has d = 0, where |d|'s central difference is 0 = sign(0).)"""
    c = BY_NAME[name]
    x, y = IC.inputs(c)
    up = np.array([1.0])
    g = IC.run_arrays(x, y, w, torch.float64)["grad"].numpy()
    x64, h, fd = x.astype(np.float64), 1e-6, np.zeros(x.shape)
    taps = torch.from_numpy(IC.header()[2]).double()

    def loss_of(a):
        xa, ya = torch.from_numpy(a), torch.from_numpy(y).double()
        d = xa - ya
        val = w[0] * d.abs().mean(dim=(1, 2, 3)) + w[1] * (d * d).mean(dim=(1, 2, 3)) + w[2] * (1 - IC.ssim_map(xa, ya, taps).mean(dim=(1, 2, 3)))
        return float((val * torch.from_numpy(up)).sum())
    for i in np.ndindex(*x.shape):
        p, m = x64.copy(), x64.copy()
        p[i] += h
        m[i] -= h
        fd[i] = (loss_of(p) - loss_of(m)) / (2 * h)
    e = np.abs(fd - g).max() / max(np.abs(g).max(), 1e-30)
    print(f"fd {name} {w}: {e:.3e}")
    assert e <= 1e-6


def test_identical_images_give_exact_zeros():
    c = BY_NAME["identical"]
    for w in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.7, 0.3, 0.0)):
        got = IC.host_run(c, w)
        assert (got["terms"][:, :2] == 0).all() and (got["terms"][:, 3] == 0).all()
        assert (got["grad"] == 0).all()
    got = IC.host_run(c, (0.0, 0.0, 1.0))
    assert np.abs(got["terms"][:, 2] - 1.0).max() <= 2.0 ** -22 and np.abs(got["map"] - 1.0).max() <= 2.0 ** -20


def test_constant_images_interior_literal():
    c = BY_NAME["constant"]
    w = (0.0, 0.0, 1.0)
    B, C, H, W = c.shape
    assert H > 12 and W > 12
    m64 = IC.reference(c, w)["o64"]["map"]
    inner = m64[:, :, 6:H - 6, 6:W - 6]
    assert abs(IC.CONST_MAP - 0.80006397953) < 1e-10
    assert (inner / IC.CONST_MAP - 1).abs().max().item() <= IC.CONST_TOL
    host = torch.from_numpy(IC.host_run(c, w)["map"])[:, :, 6:H - 6, 6:W - 6]
    assert (host.double() / IC.CONST_MAP - 1).abs().max().item() <= IC.CONST_TOL + 2.0 ** -20
    t = IC.host_run(c, (1.0, 1.0, 0.0))["terms"]
    assert t[0, 0] == np.float32(0.25) and t[0, 1] == np.float32(0.0625)


def test_clamp_mask_and_nan():
    c = BY_NAME["clamp"]
    x, y = IC.inputs(c)
    assert (x < 0).any() and (x > 1).any() and x.flat[0] == 0 and x.flat[1] == 1 and x.flat[3] == 1
    for w in ((1.0, 0.0, 0.0), (0.8, 0.0, 0.2)):
        g = IC.host_run(c, w)["grad"]
        outside = (x < 0) | (x > 1)
        assert (g[outside] == 0).all() and (g[~outside] != 0).all()       # the mask is inclusive: 0 and 1 pass
    plain = IC.host_arrays(x, y, (1.0, 0.0, 0.0), clamp=False)["grad"]
    assert (plain != 0).all()                                             # without the flag nothing is masked
    xn = x.copy()
    xn[1, 2, 3, 4] = np.nan
    g = IC.host_arrays(xn, y, (1.0, 0.0, 0.0), clamp=True)
    assert g["grad"][1, 2, 3, 4] == 0 and np.isnan(g["terms"][1]).all() and np.isfinite(g["terms"][0]).all()
    assert np.array_equal(g["grad"][0], IC.host_run(c, (1.0, 0.0, 0.0))["grad"][0])


def test_terms_do_not_depend_on_the_optional_outputs():
    c = BY_NAME["2x3x37x45"]
    x, y = IC.inputs(c)
    full = IC.host_run(c, (0.8, 0.0, 0.2))["terms"]
    assert np.array_equal(full, IC.host_arrays(x, y, (0.8, 0.0, 0.2), want_grad=False, want_map=False)["terms"])

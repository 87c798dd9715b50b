"""gsr_imgloss on the device against tests/imgloss_cases.py: terms, the SSIM map and the gradient within the project's bound
(floor 2^-22, never above 1e-3) of the float64 oracle, the margins asserted first; the map and the gradient bit for bit the
host build's (they share the per-pixel source); sentinel-filled outputs and a NaN-filled workspace change nothing; the
optional outputs, a second call, a side stream and misaligned tensors give the same bits; a NaN stays inside its image; the
clamp flag; the autograd function; the reference-named functions against the reference's recorded outputs; and the stealth
term in pgd_attack, bit for bit repeatable."""
import ctypes
import os

import numpy as np
import pytest
import torch

import imgloss_cases as IC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
CASES = IC.cases()
BY_NAME = {c.name: c for c in CASES}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_imgloss.npz")
W_MIX = (0.8, 0.0, 0.2)


@pytest.fixture(scope="module")
def IL():
    from diff_gaussian_rasterization import imgloss_ops
    assert imgloss_ops.available()
    return imgloss_ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _off4(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    k = 1 + (-(buf.data_ptr() // 4) % 4)                    # element k sits on boundary + 4
    out = buf[k:k + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def _raw(IL, x, y, w, clamp=False, grad=True, smap=True, no_grad_flag=False, stream=None, misalign=False):
    """The C call itself on sentinel-filled outputs and a NaN-filled workspace of exactly the bytes asked for."""
    from diff_gaussian_rasterization._ops_common import call, workspace, workspace_bytes
    xt, yt = (x if torch.is_tensor(x) else _t(x)), (y if torch.is_tensor(y) else _t(y))
    cs = IL.c_spec(IL.ImgLossSpec(w[0], w[1], w[2], clamp), xt.shape, IL.NO_GRAD if no_grad_flag else 0)
    n = workspace_bytes("gsr_imgloss_workspace_bytes", cs)
    ws = workspace(n, xt.device)
    ws.view(torch.float32).fill_(float("nan"))
    mk = (lambda shape: _off4(torch.full(shape, SENTINEL, dtype=torch.float32, device=xt.device))) if misalign else \
         (lambda shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=xt.device))
    if misalign:
        xt, yt = _off4(xt), _off4(yt)
    terms = mk((xt.shape[0], 4))
    g = mk(tuple(xt.shape)) if grad else None
    m = mk(tuple(xt.shape)) if smap else None
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(xt.device)):
        call("gsr_imgloss", xt.device, ctypes.byref(cs), xt.data_ptr(), yt.data_ptr(), ws.data_ptr(), n, terms.data_ptr(),
             g.data_ptr() if grad else None, m.data_ptr() if smap else None)
    torch.cuda.synchronize()
    return dict(terms=terms, grad=g, map=m)


# ---- 1. the oracle and the host build -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_device_matches_the_oracle_and_the_host_bits(IL, c):
    assert IC.margins_ok(c)
    x, y = IC.inputs(c)
    fails = []
    for w in IC.WEIGHTS:
        got = _raw(IL, x, y, w, clamp=c.clamp)
        for k in IC.COMPARED:
            assert not (got[k] == SENTINEL).any(), (k, w)                      # every element written
        fails += [(w,) + f for f in IC.check({k: v.cpu() for k, v in got.items()}, IC.reference(c, w), f"device {c.id} {w}")]
        host = IC.host_run(c, w)
        assert _bits(got["map"]) == host["map"].tobytes(), w
        assert _bits(got["grad"]) == host["grad"].tobytes(), w
        if w == (0.0, 0.0, 0.0):
            assert (got["grad"] == 0).all() and (got["terms"][:, 3] == 0).all()
    assert not fails, fails


# ---- 2. what must not matter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("2x3x37x45", CASES[4].name, "clamp"))
def test_optional_outputs_workspace_repeat_stream_and_alignment(IL, name):
    c = BY_NAME[name]
    x, y = IC.inputs(c)
    base = _raw(IL, x, y, W_MIX, clamp=c.clamp)
    spec = IL.ImgLossSpec(*W_MIX, c.clamp)
    # the binding: outputs from torch.empty, the cached workspace -- and again
    for _ in range(2):
        t, g, m = IL.imgloss_forward(_t(x), _t(y), spec, want_grad=True, want_map=True)
        assert _bits(t) == _bits(base["terms"]) and _bits(g) == _bits(base["grad"]) and _bits(m) == _bits(base["map"])
    # without the gradient, without the map, without both; with the small workspace of GSR_IMGLOSS_NO_GRAD
    for kw in (dict(grad=False), dict(smap=False), dict(grad=False, smap=False), dict(grad=False, no_grad_flag=True),
               dict(grad=False, smap=False, no_grad_flag=True)):
        got = _raw(IL, x, y, W_MIX, clamp=c.clamp, **kw)
        assert _bits(got["terms"]) == _bits(base["terms"]), kw
        if got["map"] is not None:
            assert _bits(got["map"]) == _bits(base["map"]), kw
        if got["grad"] is not None:
            assert _bits(got["grad"]) == _bits(base["grad"]), kw
    t, g, m = IL.imgloss_forward(_t(x), _t(y), spec, want_grad=False)
    assert g is None and m is None and _bits(t) == _bits(base["terms"])
    # a side stream
    side = torch.cuda.Stream(device=DEV)
    got = _raw(IL, x, y, W_MIX, clamp=c.clamp, stream=side)
    for k in IC.COMPARED:
        assert _bits(got[k]) == _bits(base[k]), k
    # every tensor 4 bytes past a 16-byte boundary
    got = _raw(IL, x, y, W_MIX, clamp=c.clamp, misalign=True)
    for k in IC.COMPARED:
        assert _bits(got[k]) == _bits(base[k]), k


def test_a_nan_stays_inside_its_image(IL):
    c = BY_NAME["2x3x37x45"]
    x, y = IC.inputs(c)
    xn = x.copy()
    xn[0, 1, 20, 30] = np.nan
    for clamp in (False, True):
        got = _raw(IL, xn, y, W_MIX, clamp=clamp)
        one = _raw(IL, x[1:], y[1:], W_MIX, clamp=clamp)
        assert torch.isnan(got["terms"][0]).all()
        assert _bits(got["terms"][1]) == _bits(one["terms"][0])
        assert _bits(got["grad"][1]) == _bits(one["grad"][0]) and _bits(got["map"][1]) == _bits(one["map"][0])
        assert torch.isfinite(got["grad"][1]).all()
        if clamp:
            assert got["grad"][0, 1, 20, 30] == 0                              # the mask: a NaN gives 0
    yn = y.copy()
    yn[1, 0, 0, 0] = np.nan                                                      # ... and in the reference image
    got = _raw(IL, x, yn, W_MIX)
    one = _raw(IL, x[:1], y[:1], W_MIX)
    assert torch.isnan(got["terms"][1]).all() and _bits(got["terms"][0]) == _bits(one["terms"][0])
    assert _bits(got["grad"][0]) == _bits(one["grad"][0])


def test_clamp_flag(IL):
    c = BY_NAME["clamp"]
    x, y = IC.inputs(c)
    got = _raw(IL, x, y, (1.0, 0.0, 0.0), clamp=True)
    outside = torch.from_numpy((x < 0) | (x > 1)).to(DEV)
    assert outside.any() and (got["grad"][outside] == 0).all() and (got["grad"][~outside] != 0).all()
    # the same call on clamped copies without the flag: the same terms and map, the gradient unmasked
    xc, yc = (np.where(a < 0, np.float32(0), np.where(a > 1, np.float32(1), a)) for a in (x, y))     # (keeps a -0)
    plain = _raw(IL, xc, yc, (1.0, 0.0, 0.0))
    assert _bits(plain["terms"]) == _bits(got["terms"]) and _bits(plain["map"]) == _bits(got["map"])
    assert torch.equal(plain["grad"][~outside], got["grad"][~outside])
    unclamped = _raw(IL, x, y, (1.0, 0.0, 0.0))
    assert _bits(unclamped["terms"]) != _bits(got["terms"])                    # without the flag nothing is clamped


# ---- 3. autograd and the public functions -----------------------------------------------------------------------------------------
def test_autograd_with_per_image_upstream_factors(IL):
    c = BY_NAME["2x3x37x45"]
    x, y = IC.inputs(c)
    up = np.array([0.25, -3.0])
    o64 = IC.run_arrays(x, y, W_MIX, torch.float64, upstream=up)
    o32 = IC.run_arrays(x, y, W_MIX, torch.float32, upstream=up)
    xt = _t(x).requires_grad_(True)
    terms, smap = IL.image_loss(xt, _t(y), *W_MIX, want_map=True)
    assert terms.shape == (2, 4) and terms.requires_grad and not smap.requires_grad
    (terms[:, 3] * _t(up.astype(np.float32))).sum().backward()
    for k, got in (("terms", terms.detach()), ("grad", xt.grad), ("map", smap)):
        e, yd = IC.err(got, o64[k]), IC.err(o32[k], o64[k])
        print(f"autograd {k}: err {e:.3e} yardstick {yd:.3e} bound {IC.bound(yd):.3e}")
        assert e <= IC.bound(yd), k
    raw = _raw(IL, x, y, W_MIX)
    assert _bits(terms) == _bits(raw["terms"])
    assert torch.equal(xt.grad, raw["grad"] * _t(up.astype(np.float32)).view(-1, 1, 1, 1))
    # the other columns carry no gradient
    xt.grad = None
    t2 = IL.image_loss(xt, _t(y), *W_MIX)
    t2[:, :3].sum().backward()
    assert xt.grad is None or (xt.grad == 0).all()
    # no gradient wanted: the small workspace path, the same terms
    with torch.no_grad():
        assert _bits(IL.image_loss(_t(x), _t(y), *W_MIX)) == _bits(raw["terms"])
    # float16 images: converted on the way in, the gradient cast back
    xh = _t(x).half().requires_grad_(True)
    IL.image_loss(xh, _t(y).half(), *W_MIX)[:, 3].sum().backward()
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape
    with pytest.raises(ValueError, match="must not require grad"):
        IL.image_loss(_t(x), _t(y).requires_grad_(True), *W_MIX)


def test_reference_named_functions_against_the_recorded_outputs(IL):
    from gsplat_attack import image_loss as GL
    c = BY_NAME["x".join(map(str, IC.GOLDEN_SHAPE))]
    with np.load(GOLDEN) as g:
        x, y = g["img"], g["ref"]
        want = {k: g[k] for k in ("l1", "l2", "ssim_mean", "ssim_per_image", "psnr")}
    xt, yt = _t(x), _t(y)
    got = dict(l1=GL.l1_loss(xt, yt), l2=GL.l2_loss(xt, yt), ssim_mean=GL.ssim(xt, yt), ssim_per_image=GL.ssim(xt, yt, size_average=False),
               psnr=GL.psnr(xt, yt))
    yard = IC.reference(c, (0.0, 0.0, 1.0))["yard"]["terms"]
    for k, w in want.items():
        e = IC.err(got[k], torch.as_tensor(w))
        print(f"fixture {k}: err {e:.3e} bound {IC.bound(yard):.3e}")
        assert tuple(got[k].shape) == tuple(np.shape(w)) and e <= IC.bound(yard), k
    # a single [C,H,W] image: scalars, and psnr per channel like the reference's view(shape[0], -1)
    assert GL.l1_loss(xt[0], yt[0]).shape == () and GL.ssim(xt[0], yt[0]).shape == () and GL.psnr(xt[0], yt[0]).shape == (3, 1)
    # the gradient of ssim is minus the stage's gradient of 1 - ssim, scaled by the mean's 1 / B
    xg = xt.clone().requires_grad_(True)
    GL.ssim(xg, yt).backward()
    raw = _raw(IL, x, y, (0.0, 0.0, 1.0))
    assert torch.equal(xg.grad, raw["grad"] * -0.5)
    # ImageLoss and photometric_loss: the batch mean of loss_b
    raw = _raw(IL, x, y, (0.8, 0.0, 0.2))
    assert torch.equal(GL.photometric_loss(xt, yt), raw["terms"][:, 3].mean())
    assert torch.equal(GL.ImageLoss(0.8, 0.0, 0.2)(xt, yt), raw["terms"][:, 3].mean())
    assert torch.equal(GL.ImageLoss(0.8, 0.0, 0.2).terms(xt, yt), raw["terms"])


# ---- 4. the stealth term in the attack --------------------------------------------------------------------------------------------
PARAMS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")


def _scene():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), width=64, height=64, n_views=2)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _attack(weight, with_term=True):
    from gsplat_attack.attack import SurrogateDetector, pgd_attack
    from gsplat_attack.image_loss import ImageLoss, with_image_term
    from gsplat_attack.renderer import PipelineParams, render
    model, cams, bg = _scene()
    det = SurrogateDetector().to(DEV)
    loss_fn = det
    if with_term:
        with torch.no_grad():
            refs = torch.stack([render(c, model, PipelineParams(skip_objects=True), bg)["render"] for c in cams])
        loss_fn = with_image_term(det, refs, ImageLoss(0.8, 0.0, 0.2), weight)
    hist = pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=True, loss_fn=loss_fn)
    torch.cuda.synchronize()
    return hist, [model.named_parameters()[n].detach().clone() for n in PARAMS]


def test_pgd_attack_with_the_image_term_repeats():
    h0, p0 = _attack(0.0, with_term=False)
    ha, pa = _attack(50.0)
    hb, pb = _attack(50.0)
    hz, pz = _attack(0.0)
    assert len(ha) == 2 and all(np.isfinite(v) for v in ha)
    assert ha == hb and all(torch.equal(a, b) for a, b in zip(pa, pb))         # two runs: the same bits
    assert any(not torch.equal(a, b) for a, b in zip(pa, p0))                  # the term moved the parameters
    assert hz == h0 and all(torch.equal(a, b) for a, b in zip(pz, p0))         # weight 0: the run without the term

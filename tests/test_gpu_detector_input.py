"""The image front end on the device: the kernels bit for bit the host build of the same source
(tests/host_math/image_host.cpp, itself within derived bounds of F.interpolate: tests/test_image_host_cpu.py), the uint8
conversion against its torch expression, autograd through the Python surface against the float64 CPU composition, and a
render -> letterbox -> detector -> backward chain that repeats bit for bit."""
import numpy as np
import pytest
import torch

import image_cases as IC
from image_cases import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def host():
    return IC.host_lib()


@pytest.fixture(scope="module")
def IO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import image_ops
    D._load()
    assert image_ops.available()
    return image_ops


def _spec(IO, c: Case):
    return IO.ResampleSpec(c.oh, c.ow, c.rh, c.rw, c.top, c.left, c.pad, c.mean, c.inv_std, c.clamp)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("c", IC.RESIZES + IC.COMPOSED + IC.GPU_EXTRA, ids=lambda c: c.id)
def test_kernels_bit_for_bit_the_host_build(host, IO, c):
    src, g = IC.make_inputs(c)
    spec = _spec(IO, c)
    x = torch.from_numpy(src).to(DEV)
    out = IO.resample(x, spec)
    assert np.array_equal(_bits(out), IC.host_forward(host, c, src).view(np.uint32))
    gd = torch.from_numpy(g).to(DEV)
    # the destination was filled with NaN first: every source pixel is written, none is left as it was
    first = IO.resample_backward(gd, spec, x.shape, src=x, out=torch.full_like(x, float("nan")))
    want, _ = IC.host_backward(host, c, src, g)
    assert np.array_equal(_bits(first), want.view(np.uint32))
    again = IO.resample_backward(gd, spec, x.shape, src=x)
    assert np.array_equal(_bits(again), _bits(first))
    # accumulate = 1 onto a base, against the host's accumulate
    base = np.random.default_rng(3).standard_normal(src.shape).astype(np.float32)
    acc = IO.resample_backward(gd, spec, x.shape, src=x, out=torch.from_numpy(base).to(DEV), accumulate=True)
    assert np.array_equal(_bits(acc), IC.host_backward(host, c, src, g, into=base)[0].view(np.uint32))


def test_unaligned_views_take_the_scalar_stores(host, IO):
    """W % 4 == 0 but the gradient buffer starts 4 bytes off a 16-byte boundary: the 4-byte-store kernel, same bits."""
    c = Case(12, 20, 24, 40, clamp=True)
    src, g = IC.make_inputs(c)
    spec = _spec(IO, c)
    x = torch.from_numpy(src).to(DEV)
    flat = torch.full((src.size + 1,), float("nan"), device=DEV)
    out = flat[1:].view(src.shape)
    assert out.data_ptr() % 16 == 4
    IO.resample_backward(torch.from_numpy(g).to(DEV), spec, x.shape, src=x, out=out)
    assert np.array_equal(_bits(out), IC.host_backward(host, c, src, g)[0].view(np.uint32))
    assert torch.isnan(flat[0])


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 64, 1921), (2, 3, 8, 64)])
def test_to_uint8_hwc(IO, shape):
    n = int(np.prod(shape))
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    special = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                              np.array([0.0, 1.0, -0.0], np.float32)]).astype(np.float32)
    vals = np.random.default_rng(n).uniform(-0.2, 1.2, n).astype(np.float32)
    m = min(n, special.size)
    vals[np.random.default_rng(1).permutation(n)[:m]] = special[:m]
    # the small shape: the remaining specials in further tensors of the same shape
    xs = [vals] + [np.resize(special[i:i + n], n).astype(np.float32) for i in range(m, special.size, n)]
    for v in xs:
        x = torch.from_numpy(v.reshape(shape)).to(DEV)
        got = IO.to_uint8_hwc(x)
        want = (x.clamp(0, 1) * 255).byte().permute(0, 2, 3, 1).contiguous()
        assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got, want)
    one = IO.to_uint8_hwc(x[0])
    assert torch.equal(one, want[0])
    assert int(IO.to_uint8_hwc(torch.full((1, 3, 2, 2), float("nan"), device=DEV)).max()) == 0


def _autograd_case(fn, c: Case):
    """fn(x on the device) through autograd against the float64 CPU composition of `c`, within the derived bounds."""
    src, g = IC.make_inputs(c)
    x = torch.from_numpy(src).to(DEV).requires_grad_(True)
    out = fn(x)
    assert tuple(out.shape) == (c.B, c.C, c.oh, c.ow)
    out.backward(torch.from_numpy(g).to(DEV))
    ref, gref, fb, bb = IC.oracle(c, src, g)
    _, n_max = IC.host_backward(IC.host_lib(), c, src, g)
    err = float(np.abs(out.detach().cpu().numpy().astype(np.float64) - ref).max())
    gerr = float(np.abs(x.grad.cpu().numpy().astype(np.float64) - gref).max())
    print(f"{c.id}: forward err {err:.3e} bound {fb:.3e}; backward err {gerr:.3e} bound {bb(n_max):.3e}")
    assert err <= fb and gerr <= bb(n_max)


def test_letterbox_autograd():
    from gsplat_attack import detector_input as DI
    c = Case(54, 96, 27, 48, 48, 48, 10, 0, 114 / 255, B=2)
    seen = {}

    def fn(x):
        img, seen["scale"], seen["left"], seen["top"] = DI.letterbox(x, (48, 48))
        return img
    _autograd_case(fn, c)
    assert seen == {"scale": 0.5, "left": 0, "top": 10}
    _autograd_case(lambda x: DI.DetectorInput(letterbox=(48, 48), clamp=True)(x), c._replace(clamp=True))


def test_resize_shorter_side_and_multiple_autograd():
    from gsplat_attack import detector_input as DI
    c = Case(27, 48, 40, 71, **IC.IMAGENET)            # int(40 * 48 / 27) = 71
    _autograd_case(lambda x: DI.resize_shorter_side(x, 40, **IC.IMAGENET), c)
    _autograd_case(lambda x: DI.resize_to_multiple(x, 32), Case(27, 48, 32, 64))


def _scene_and_bg():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), n_views=3)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def test_render_letterbox_detector_backward_repeats_bit_for_bit():
    from gsplat_attack import detector_input as DI
    from gsplat_attack.attack import SurrogateDetector
    from gsplat_attack.renderer import PipelineParams, render_batch
    model, cams, bg = _scene_and_bg()
    det = SurrogateDetector().to(DEV)
    runs = []
    raw = [model.named_parameters()[n] for n in ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")]
    for _ in range(2):
        model.zero_grad()
        renders = render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"]
        img, _, _, _ = DI.letterbox(renders, (96, 96))
        assert tuple(img.shape) == (3, 3, 96, 96)
        det(img).backward()
        runs.append([p.grad.detach().clone() for p in raw])
    torch.cuda.synchronize()
    assert len(runs[0]) == 6
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0
        assert torch.equal(a, b)


def test_pgd_attack_through_the_detector_input_repeats():
    from gsplat_attack.attack import SurrogateDetector, pgd_attack
    from gsplat_attack.detector_input import DetectorInput, with_detector_input
    hists = []
    for _ in range(2):
        model, cams, bg = _scene_and_bg()
        loss_fn = with_detector_input(SurrogateDetector().to(DEV), DetectorInput(letterbox=(96, 96)))
        hists.append(pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=True, loss_fn=loss_fn))
    assert len(hists[0]) == 2 and all(np.isfinite(h) for h in hists[0])
    assert hists[0] == hists[1]
    assert hists[0][0] != hists[0][1]                  # the step moved the loss: the gradient got through the letterbox

"""distCUDA2 on the HIP path (gsr_knn_dist2: csrc/gsr_knn.h, csrc/gsr_knn.hip.h) against the float64 oracle of
tests/knn_cases.py, at relative 16 * 2^-24 with no absolute term, on named cases that reach every path of the search (the host
build's finish codes prove which: tests/test_knn_host_cpu.py), and against the host build of the same scalar source."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import knn_cases as KC

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def _device_result(name):
    from simple_knn._C import distCUDA2
    out = distCUDA2(_dev(KC.points(name))).cpu().numpy()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("kind", ["uniform", "city", "flat", "duplicates", "outliers", "tiny"])
def test_matches_brute_force(kind):
    from simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(sum(map(ord, kind)))   # str hashes change per process
    if kind == "uniform":
        pts = torch.rand(6000, 3, generator=g) * 10
    elif kind == "city":
        from gsplat_attack.scenes import city
        pts = city(8000, 3, 20.0, 60)["xyz"]
    elif kind == "flat":                      # a degenerate bounding box (all z equal)
        pts = torch.rand(3000, 3, generator=g)
        pts[:, 2] = 0.25
    elif kind == "duplicates":                # coincident points: zero distances count
        base = torch.rand(500, 3, generator=g)
        pts = torch.cat([base, base[:200], base[:50]])
    elif kind == "outliers":                  # isolated points far from a dense cluster
        pts = torch.cat([torch.randn(4000, 3, generator=g) * 0.1, torch.randn(12, 3, generator=g) * 500])
    else:
        pts = torch.rand(7, 3, generator=g)
    pts = pts.float().contiguous().cpu()
    got = distCUDA2(pts.cuda()).cpu().numpy()
    ref = KC.oracle_rows(pts.numpy(), np.arange(len(pts)))
    w = KC.worst_ratio(got, ref)
    print(f"knn device {kind}: P {len(pts)} worst error / bound {w:.3f}")
    assert w <= 1.0, (kind, w)


@pytest.mark.parametrize("name", KC.NAMES)
def test_case_matches_oracle(name):
    """every named case; 'slabs' on the oracle's sample, which holds every point the host build sends to the full sweep"""
    got = _device_result(name)
    assert got.shape == (len(KC.points(name)),)
    KC.check("device", name, got[KC.sample_rows(name)], KC.oracle(name))


@pytest.mark.parametrize("name", KC.NAMES)
def test_case_matches_host_build(name):
    """the same scalar source through g++: floats within the tolerance (the device may contract the squared distance into
    FMAs, the host build does not), zeros and infinities at the same points"""
    host = KC.host_result(name)[0]
    KC.check("device vs host", name, _device_result(name), host.astype(np.float64))


def test_fewer_than_four_points_on_the_device():
    for name in ("p1", "p2"):
        assert np.isposinf(_device_result(name)).all()
    assert np.array_equal(_device_result("p3"), np.full(3, KC.FLT_MAX / np.float32(3.0), np.float32))


def test_poisoned_points_on_the_device():
    for name, at in (("nan-point", KC.NAN_AT), ("inf-point", KC.INF_AT)):
        got = _device_result(name)
        keep = np.arange(len(got)) != at[0]
        assert got[at[0]] == np.inf and np.isfinite(got[keep]).all()
        KC.check("device finite subset", name, got[keep], KC.oracle_rows(KC.points(name)[keep], np.arange(keep.sum())))


@pytest.mark.parametrize("name", KC.NAMES)
def test_repeat_and_side_stream_give_the_same_bits(name):
    """the only atomics are the bounding box's min / max, which do not depend on order"""
    from simple_knn._C import distCUDA2
    pts = _dev(KC.points(name))
    first = _device_result(name).view(np.uint32)
    again = distCUDA2(pts).cpu().numpy().view(np.uint32)
    assert np.array_equal(again, first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = distCUDA2(pts)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), first)


@pytest.mark.parametrize("name", ["p1", "p3", "p7", "uniform", "slabs", "inf-point"])
def test_nothing_is_written_outside_the_output(name):
    import diff_gaussian_rasterization as D
    lib = D._load()
    pts = _dev(KC.points(name))
    P, pad = pts.shape[0], 64
    buf = torch.full((P + 2 * pad,), -7.0, dtype=torch.float32, device="cuda")
    rc = lib.gsr_knn_dist2(pts.data_ptr(), P, buf.data_ptr() + 4 * pad, D._stream(pts.device))
    assert rc == 0, D._err(lib)
    torch.cuda.synchronize()
    buf = buf.cpu().numpy()
    assert (buf[:pad] == -7.0).all() and (buf[pad + P:] == -7.0).all()
    assert np.array_equal(buf[pad:pad + P].view(np.uint32), _device_result(name).view(np.uint32))


def test_strided_and_half_inputs_go_through_the_shim():
    from simple_knn._C import distCUDA2
    base = KC.points("uniform")
    wide = torch.zeros(len(base), 6)
    wide[:, ::2] = torch.from_numpy(np.array(base))
    strided = wide.cuda()[:, ::2]
    assert not strided.is_contiguous()
    assert np.array_equal(distCUDA2(strided).cpu().numpy().view(np.uint32), _device_result("uniform").view(np.uint32))
    half = torch.from_numpy(np.array(base)).half()
    got = distCUDA2(half.cuda())
    assert got.dtype == torch.float32
    w = KC.worst_ratio(got.cpu().numpy(), KC.oracle_rows(half.float().numpy(), np.arange(len(base))))
    print(f"knn device half input: worst error / bound {w:.3f}")
    assert w <= 1.0


def test_no_points():
    from simple_knn._C import distCUDA2
    out = distCUDA2(torch.zeros(0, 3, device="cuda"))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.is_cuda


@pytest.mark.parametrize("P", [3, 5])
def test_create_from_pcd_gives_the_same_scales_on_either_device(P):
    """below 4 points the CPU branch follows the kernel's contract (FLT_MAX for a missing neighbour).  atol: the two paths'
    d^2 differ by at most 2 * 16 * 2^-24, which log sqrt halves (1e-6), plus 2 ulp of a float32 log of magnitude <= 44.4
    (7.6e-6)"""
    from gsplat_attack.gaussian_model import GaussianModel
    pts = torch.from_numpy(np.array(KC.points(f"p{P}")))
    cols = torch.rand(P, 3, generator=torch.Generator().manual_seed(P))
    dev = GaussianModel.create_from_pcd(pts, cols, device=torch.device("cuda:0"))
    cpu = GaussianModel.create_from_pcd(pts, cols, device="cpu")
    a, b = dev._scaling.detach().cpu(), cpu._scaling.detach()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.allclose(a, b, rtol=0, atol=1e-5), (a, b)
    if P == 3:
        assert torch.allclose(b, torch.full_like(b, 0.5 * float(np.log(np.float64(KC.FLT_MAX) / 3.0))), rtol=0, atol=1e-5)


def test_one_million_points_runs_and_is_plausible():
    """the only run with more than 262 144 points: the bounding-box kernel's grid-stride loop"""
    from simple_knn._C import distCUDA2
    from gsplat_attack.scenes import city
    pts = city(1_000_000, 3, 20.0, 60)["xyz"].cuda()
    d = distCUDA2(pts)
    assert d.shape == (1_000_000,) and torch.isfinite(d).all() and float(d.min()) >= 0
    # spot check 200 random points against brute force from coordinate differences in float64
    idx = torch.randperm(1_000_000, generator=torch.Generator().manual_seed(0))[:200].cuda()
    x = pts.double()
    ref = []
    for s in range(0, 200, 50):
        r = idx[s:s + 50]
        d2 = torch.zeros(len(r), x.shape[0], dtype=torch.float64, device=x.device)
        for a in range(3):
            d2 += (x[r, a][:, None] - x[None, :, a]).square_()
        d2[torch.arange(len(r)), r] = float("inf")
        ref.append(torch.topk(d2, 3, dim=1, largest=False).values.sum(dim=1) / 3.0)
    w = KC.worst_ratio(d[idx].cpu().numpy(), torch.cat(ref).cpu().numpy())
    print(f"knn device 1M spot check: worst error / bound {w:.3f}")
    assert w <= 1.0


def test_model_from_colmap_points_renders():
    """COLMAP sparse points -> create_from_pcd (distCUDA2 on the HIP path) -> render(): the data-format side of the
    path end to end on the device."""
    import os
    from gsplat_attack.colmap import cameras_from_colmap, read_points3D_binary
    from gsplat_attack.gaussian_model import GaussianModel
    from gsplat_attack.renderer import PipelineParams, render
    here = os.path.dirname(os.path.abspath(__file__))
    xyz, rgb, _ = read_points3D_binary(os.path.join(here, "golden", "colmap_sample_bin", "sparse", "0", "points3D.bin"))
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    pts = torch.cat([torch.from_numpy(xyz).float(), torch.randn(2000, 3, generator=g) * 0.5])
    cols = torch.cat([torch.from_numpy(rgb).float() / 255.0, torch.rand(2000, 3, generator=g)])
    model = GaussianModel.create_from_pcd(pts, cols, device=dev)
    cpu = GaussianModel.create_from_pcd(pts, cols, device="cpu")
    assert torch.allclose(model._scaling.detach().cpu(), cpu._scaling.detach(), atol=1e-4)
    cam = cameras_from_colmap(os.path.join(here, "golden", "colmap_sample_bin"), device=dev)[0]
    out = render(cam, model, PipelineParams(), torch.zeros(3, device=dev))
    out["render"].sum().backward()
    torch.cuda.synchronize()
    assert out["render"].shape == (3, cam.image_height, cam.image_width) and torch.isfinite(out["render"]).all()
    assert torch.isfinite(model._xyz.grad).all()

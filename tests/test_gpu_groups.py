"""Groups mode on the device (C ABI 603): the classification kernel against a float64 softmax(conv1x1), the hull inclusion
kernel against the same planes evaluated in numpy float64, select_group end to end on S-nyc-1M with a closed-form
answer and its peak device memory, split_group + render_pair against the unsplit render, and three PGD steps of a
groups-mode attack."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MB = 1 << 20


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ref_psel(f, W, b, ids):
    logits = f.double() @ W.double().T + b.double()
    return torch.softmax(logits, dim=1)[:, list(ids)].max(dim=1).values


@pytest.mark.parametrize("C,idsets", [(1, [[0]]), (17, [[3], [0, 16], [5, 9, 2], [1, 4, 7, 11]]),
                                      (256, [[117], [0, 255], [10, 20, 30], [117, 3, 64, 200]])])
def test_classify_kernel_against_float64(dev, C, idsets):
    from diff_gaussian_rasterization import groups as G
    g = torch.Generator().manual_seed(C)
    P = 100_000
    f = torch.randn(P, 1, 16, generator=g) * 0.7
    W = torch.randn(C, 16, generator=g) * 0.8
    b = torch.randn(C, generator=g) * 0.5
    fd, Wd, bd = f.to(dev), W.to(dev), b.to(dev)
    for ids in idsets:
        ref = _ref_psel(f.reshape(P, 16), W, b, ids)
        thresh = 0.5 if C == 1 else float(torch.quantile(ref.float(), 0.6))
        mask, psel = G.group_classify(fd, Wd, bd, ids, thresh)
        err = (psel.double().cpu() - ref).abs().max().item()
        assert err <= 1e-6, (C, ids, err)
        want = ref > thresh
        sure = (ref - thresh).abs() > 1e-6
        assert torch.equal(mask.cpu()[sure], want[sure]), (C, ids)
        assert 0 < int(want.sum()) <= P
        mask2, psel2 = G.group_classify(fd, Wd, bd, ids, thresh)
        assert torch.equal(psel, psel2) and torch.equal(mask, mask2)            # bitwise reproducible
        print(f"[classify C={C} ids={ids}] max |psel - float64| {err:.2e}, selected {int(mask.sum())}")


def _np_inside(planes, bbox, tau, q):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    inbox = np.all((q >= bbox[:3] - tau) & (q <= bbox[3:] + tau), axis=1)
    if len(planes) == 0:
        return np.zeros(len(q), bool)
    s = planes[None, :, 0] * q[:, 0:1]
    s = s + planes[None, :, 1] * q[:, 1:2]
    s = s + planes[None, :, 2] * q[:, 2:3]
    return inbox & np.all(s - planes[None, :, 3] <= tau, axis=1)


def test_inclusion_kernel_against_numpy(dev):
    from diff_gaussian_rasterization import groups as G
    cube = np.array([[x, y, z] for x in (1.0, 2.0) for y in (1.0, 2.0) for z in (1.0, 2.0)])
    h = G.convex_hull_planes(cube)
    assert len(h.planes) == 12 and not h.degenerate
    # face centres at +-1e-4, the faces themselves, one float32 step outside them, and a cloud around the cube
    q = []
    for axis in range(3):
        for side, away in ((1.0, 0.0), (2.0, 3.0)):
            for d in (-1e-4, 1e-4, 0.0):
                p = np.full(3, 1.5); p[axis] = side + d
                q.append(p)
            p = np.full(3, 1.5); p[axis] = np.nextafter(np.float32(side), np.float32(away))
            q.append(p)
    rng = np.random.default_rng(0)
    q = np.concatenate([np.array(q), rng.uniform(0.8, 2.2, size=(200_000, 3)),
                        np.round(rng.uniform(0.9, 2.1, size=(50_000, 3)) * 8) / 8])   # many exactly on faces and edges
    q32 = q.astype(np.float32)
    xyz = torch.from_numpy(q32).to(dev)
    got = G.points_in_hull(xyz, h).cpu().numpy()
    want = _np_inside(h.planes, h.bbox, h.tau, q32)
    assert np.array_equal(got, want)
    face = got[:24].reshape(6, 4)                                 # per face: -1e-4, +1e-4, on the face, one step out
    assert face[:, 2].all() and not face[:, 3].any()
    assert face[0::2, 1].all() and not face[0::2, 0].any()        # lower faces: +1e-4 is inside
    assert face[1::2, 0].all() and not face[1::2, 1].any()        # upper faces: -1e-4 is inside
    # tau itself: a tolerance of 0.01 takes in points 0.005 beyond a face and not 0.02 beyond
    wide = G.Hull(h.planes, h.bbox, 0.01, False)
    t = torch.tensor([[2.005, 1.5, 1.5], [1.5, 0.995, 1.5], [2.02, 1.5, 1.5], [1.5, 1.5, 0.98]], device=dev)
    assert G.points_in_hull(t, wide).tolist() == [True, True, False, False]
    # a random hull, and the fused OR with a mask
    blob = rng.normal(size=(60, 3)) * [1.0, 2.0, 0.5]
    hb = G.convex_hull_planes(blob)
    qb = (rng.normal(size=(300_000, 3)) * [1.0, 2.0, 0.5] * 1.2).astype(np.float32)
    mask = torch.from_numpy(rng.uniform(size=300_000) < 0.1).to(dev)
    got = G.points_in_hull(torch.from_numpy(qb).to(dev), hb, mask_in=mask).cpu().numpy()
    want = _np_inside(hb.planes, hb.bbox, hb.tau, qb) | mask.cpu().numpy()
    assert np.array_equal(got, want)
    # a degenerate hull selects nothing beyond the mask
    flat = G.convex_hull_planes(np.c_[rng.normal(size=(20, 2)), np.zeros(20)])
    assert flat.degenerate
    assert torch.equal(G.points_in_hull(torch.from_numpy(qb).to(dev), flat, mask_in=mask), mask)


BOX_LO, BOX_HI = (-6.0, -3.0, 1.0), (2.0, 5.0, 20.0)


@pytest.fixture(scope="module")
def grouped_city(dev):
    """S-nyc-1M with an object of class 117 in the box B: 70 % of the Gaussians inside B labelled, their positions
    redrawn uniformly in B and eight of them on B's corners (the hull of the labelled ones is B itself)."""
    from gsplat_attack.scenes import make_scene, synthetic_grouping
    model, cams, _ = make_scene("nyc-1M", device=dev, n_views=2)
    lo, hi = torch.tensor(BOX_LO, device=dev), torch.tensor(BOX_HI, device=dev)
    g = torch.Generator(device="cpu").manual_seed(117)
    with torch.no_grad():
        xyz = model._xyz
        inB = ((xyz >= lo) & (xyz <= hi)).all(dim=1)
        lab = inB & (torch.rand(xyz.shape[0], generator=g).to(dev) < 0.7)
        idx = torch.nonzero(lab).flatten()
        u = torch.rand(idx.numel(), 3, generator=g).to(dev)
        xyz[idx] = lo + u * (hi - lo)
        corners = torch.tensor([[a, b, c] for a in (BOX_LO[0], BOX_HI[0]) for b in (BOX_LO[1], BOX_HI[1])
                                for c in (BOX_LO[2], BOX_HI[2])], device=dev)
        xyz[idx[:8]] = corners
    sd = synthetic_grouping(model, lab, 117)
    return model, cams, sd, lab


def test_select_group_closed_form(dev, grouped_city):
    from gsplat_attack.groups import select_group
    model, _, sd, lab = grouped_city
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    mask3d, info = select_group(model, sd, [117], select_thresh=0.5, outlier_factor=1.0)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - base
    xyz = model._xyz.detach().double()
    lo, hi = torch.tensor(BOX_LO, device=dev).double(), torch.tensor(BOX_HI, device=dev).double()
    inB = ((xyz >= lo) & (xyz <= hi)).all(dim=1)
    D = float((hi - lo).norm())
    near = ((xyz - lo).abs().min(dim=1).values <= 1e-6 * D) | ((xyz - hi).abs().min(dim=1).values <= 1e-6 * D)
    near &= ((xyz >= lo - 1e-6 * D) & (xyz <= hi + 1e-6 * D)).all(dim=1)
    keep = ~near
    print(f"[select S-nyc-1M] {info}; inside B {int(inB.sum())}, labelled {int(lab.sum())}, near B's faces (left out) "
          f"{int(near.sum())}, peak extra device memory {extra / MB:.1f} MB")
    assert info["classified"] == int(lab.sum()) and info["hull_points"] == int(lab.sum())
    assert info["facets"] >= 12 and not info["degenerate"]      # B's six faces (a face may hold more than 2 triangles)
    assert int((inB & ~lab).sum()) > 1000                          # the hull really adds the unlabelled 30 %
    assert torch.equal(mask3d[keep], inB[keep])
    assert bool(mask3d[lab].all())
    assert extra <= 32 * MB, f"select_group used {extra / MB:.1f} MB of extra device memory"


def test_split_and_render_pair(dev, grouped_city):
    from gsplat_attack.groups import select_group, split_group
    from gsplat_attack.renderer import PipelineParams, render, render_pair
    model, cams, sd, _ = grouped_city
    mask3d, _ = select_group(model, sd, [117])
    group, rest = split_group(model, mask3d)
    assert group._xyz.shape[0] == int(mask3d.sum()) and rest._xyz.shape[0] == model._xyz.shape[0] - group._xyz.shape[0]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = PipelineParams(skip_objects=True)
    with torch.no_grad():
        full = render(cams[0], model, pipe, bg)
        pair = render_pair(cams[0], group, rest, pipe, bg)
    err = (full["render"] - pair["render"]).abs().max().item()
    print(f"[split + render_pair] max |pair - unsplit| {err:.2e}")
    assert err <= 1e-6
    order = torch.cat([torch.nonzero(mask3d).flatten(), torch.nonzero(~mask3d).flatten()])
    assert torch.equal(pair["radii"], full["radii"][order])
    assert int((pair["radii"][:group._xyz.shape[0]] > 0).sum()) > 0


def test_groups_mode_pgd(dev):
    from gsplat_attack.attack import run_attack
    from gsplat_attack.groups import select_group, split_group
    from gsplat_attack.renderer import PipelineParams, render_pair
    from gsplat_attack.scenes import make_scene, synthetic_grouping
    model, cams, _ = make_scene("nyc-1M", device=dev, P=200_000, width=480, height=272, n_views=1)
    xyz = model._xyz.detach()
    box = ((xyz[:, 0].abs() < 8) & (xyz[:, 1].abs() < 8) & (xyz[:, 2] > 0.5)).cpu()
    sd = synthetic_grouping(model, box, 42)
    mask3d, info = select_group(model, sd, [42])
    group, rest = split_group(model, mask3d)
    g0 = {n: getattr(group, n).detach().clone() for n in group._PARAM_ATTRS}
    r0 = {n: getattr(rest, n).detach().clone() for n in rest._PARAM_ATTRS}
    bg = torch.zeros(3, device=dev)
    shots = []

    def success_fn(img, j):
        shots.append(img.detach().clone())
        return False

    eps = 0.05
    out = run_attack(group, cams, background=rest, batch_size=1, max_iters=4, success_fn=success_fn, alpha=0.5,
                     epsilon=eps, groups=("color",), norm="l2", bg=bg)
    assert out["iterations"] == 4 and out["batches"][0]["iters"] == 3 and len(shots) == 3
    for n in rest._PARAM_ATTRS:
        assert torch.equal(getattr(rest, n).detach(), r0[n]), f"background {n} changed"
    for n in ("_xyz", "_scaling", "_rotation", "_opacity", "_objects_dc"):
        assert torch.equal(getattr(group, n).detach(), g0[n]), f"group {n} changed"
    moved = 0.0
    for n in ("_features_dc", "_features_rest"):
        d = (getattr(group, n).detach() - g0[n]).reshape(g0[n].shape[0], -1).double().norm(dim=1)
        assert float(d.max()) <= eps * (1 + 1e-5), (n, float(d.max()))
        moved = max(moved, float(d.max()))
    assert moved > 0.0
    with torch.no_grad():
        again = render_pair(cams[0], group, rest, PipelineParams(skip_objects=True), bg)["render"]
    print(f"[groups PGD] {info}; largest row step {moved:.4f} (eps {eps}); last success render vs render_pair: "
          f"{(shots[-1] - again).abs().max().item():.2e}")
    assert torch.equal(shots[-1], again)

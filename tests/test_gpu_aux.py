"""Depth and alpha maps from the compositors (include/gsraster.h, "Depth and alpha maps"): out_alpha = 1 - T_final,
out_depth = sum of z_i alpha_i T_i, and their backward, against oracle-R.

The oracle needs no depth output of its own: a second differentiable call with colors_precomp = (z, 1, 0) on a black
background, z = ([means3D, 1] @ viewmatrix)[:, 2] in float64 with autograd, gives the reference depth map in channel 0
and the reference alpha map in channel 1; one loss  sum g_C . C + g_D D + g_A A  over the solid pixels, one backward()
through both oracle calls.  Tolerances: alpha lives in [0, 1) like a colour -> the project's 1e-4; depth is a colour
channel scaled by z -> 1e-4 * z_far, z_far = largest float64 view depth of a Gaussian with radius > 0; gradients 1e-3
normwise plus the element criterion (util.grad_error); fragile-pixel share capped at check()'s 5e-3 for S-hydrant-1k.
"""
import copy
import math
import os

import pytest
import torch

from oracle import oracle_r as O
from util import settings_for, model_inputs, grad_error, pixel_yardstick, yardstick_line
from test_gpu_parity import hip_depth_keys, NEITHER_CAP, NEITHER_MIN_PX, RGB_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

FRAG_CAP = 5e-3            # tests/test_gpu_parity.py::check, frag_frac for this scene
SPLIT_TOL = 2e-5           # tests/test_gpu_segments.py: split / segment forms, relative to the tensor's largest gradient
RAW = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _D():
    import diff_gaussian_rasterization as D
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    D._load()
    return D


def _scene(key="hydrant-1k", **kw):
    from gsplat_attack.scenes import make_scene
    return make_scene(key, **kw)


def _act_raw(L):
    """The getters of the reference model (scene/gaussian_model.py:97-124) on raw leaves, in the leaves' dtype."""
    return dict(means3D=L["_xyz"], shs=torch.cat([L["_features_dc"], L["_features_rest"]], dim=1),
                opacities=torch.sigmoid(L["_opacity"]), scales=torch.exp(L["_scaling"]),
                rotations=torch.nn.functional.normalize(L["_rotation"]))


def oracle_aux(leaves, act, st, keys, dtype=torch.float64, tile_windows=None):
    """-> (colour RenderOut, aux RenderOut (channel 0 depth, 1 alpha), leaves incl. 'means2D', z_far)."""
    L = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in leaves.items() if v is not None}
    a = act(L)
    m2d = torch.zeros(a["means3D"].shape[0], 3, dtype=torch.float64, requires_grad=True)
    V = st.viewmatrix.detach().cpu().double()
    z = (torch.cat([a["means3D"], torch.ones_like(a["means3D"][:, :1])], dim=1) @ V)[:, 2]
    col = O.rasterize(a["means3D"], m2d, a["opacities"], st, shs=a["shs"], scales=a["scales"], rotations=a["rotations"],
                      dtype=dtype, depth_key=keys, tile_windows=tile_windows)
    st0 = st._replace(bg=torch.zeros(3))
    zc = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], dim=1)
    aux = O.rasterize(a["means3D"], m2d, a["opacities"], st0, colors_precomp=zc, scales=a["scales"],
                      rotations=a["rotations"], dtype=dtype, depth_key=keys, tile_windows=tile_windows)
    L["means2D"] = m2d
    seen = col.radii > 0
    z_far = float(z.detach()[seen].max()) if bool(seen.any()) else 1.0
    return col, aux, L, z_far


def _grads_of(loss, L):
    gs = torch.autograd.grad(loss, list(L.values()), retain_graph=True, allow_unused=True)
    return {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(L.items(), gs)}


def hip_classic(D, inp, cam, bg, dev):
    leaf = {k: v.detach().to(dev).float().clone().requires_grad_(True) for k, v in inp.items()}
    m2d = torch.zeros(leaf["means3D"].shape[0], 3, device=dev, requires_grad=True)
    st = settings_for(cam, bg, cls=D.GaussianRasterizationSettings, device=dev)
    out = D.GaussianRasterizer(raster_settings=st)(means3D=leaf["means3D"], means2D=m2d, opacities=leaf["opacities"],
                                                   shs=leaf["shs"], scales=leaf["scales"], rotations=leaf["rotations"],
                                                   aux=True)
    leaf["means2D"] = m2d
    return out, leaf


def hip_raw(D, model, cam, bg, dev, aux=True, flags=0):
    leaf = {k: getattr(model, k).detach().to(dev).float().clone().requires_grad_(True) for k in RAW}
    m2d = torch.zeros(leaf["_xyz"].shape[0], 3, device=dev, requires_grad=True)
    st = settings_for(cam, bg, cls=D.GaussianRasterizationSettings, device=dev)
    with D.extra_flags(flags):
        out = D.rasterize_gaussians_raw(leaf["_xyz"], m2d, leaf["_features_dc"], leaf["_features_rest"], None,
                                        leaf["_opacity"], leaf["_scaling"], leaf["_rotation"], st, aux=aux)
    leaf["means2D"] = m2d
    return out, leaf


def _three_losses(H, W, seed=7):
    g = torch.Generator().manual_seed(seed)
    gC, gD, gA = torch.randn(3, H, W, generator=g), torch.randn(H, W, generator=g), torch.randn(H, W, generator=g)
    z3, z1 = torch.zeros(3, H, W), torch.zeros(H, W)
    return {"all": (gC, gD, gA), "depth": (z3, gD, z1), "alpha": (z3, z1, gA)}


def _compare(tag, hip_out, hip_leaf, col, aux, L, z_far, r32, losses, solid, dev, colour_names, yard_mask=None):
    color, _, _, depth, alpha = hip_out
    A, Dm = alpha.detach().cpu()[0].double(), depth.detach().cpu()[0].double()
    eA = (A - aux.color[1].detach()).abs()[solid].max().item()
    eD = (Dm - aux.color[0].detach()).abs()[solid].max().item() / z_far
    eC = (color.detach().cpu().double() - col.color.detach()).abs().amax(dim=0)[solid].max().item()
    c32, a32 = r32
    fA = (a32.color[1].double() - aux.color[1].detach()).abs()[solid].max().item()
    fD = (a32.color[0].double() - aux.color[0].detach()).abs()[solid].max().item() / z_far
    print(f"[{tag}] z_far {z_far:.3f}  solid err: alpha {eA:.2e} (f32 oracle {fA:.2e}), depth/z_far {eD:.2e} (f32 oracle {fD:.2e}), rgb {eC:.2e}")
    hip2 = torch.stack([Dm / z_far, A])
    y = pixel_yardstick(hip2, torch.stack([aux.color[0].detach() / z_far, aux.color[1].detach()]),
                        torch.stack([a32.color[0].double() / z_far, a32.color[1].double()]),
                        col.fragile_px | aux.fragile_px, mask=yard_mask, tol=RGB_TOL)
    print(yardstick_line(tag, y))
    assert eA <= RGB_TOL and eD <= RGB_TOL and eC <= RGB_TOL
    assert y["neither_solid"] == 0
    assert y["neither_px"] <= max(NEITHER_MIN_PX, NEITHER_CAP * y["fragile"] * y["n"]), yardstick_line(tag, y)
    m = solid.double()
    for name, (gC, gD, gA) in losses.items():
        ref_loss = ((col.color * gC.double()).sum(0) * m).sum() + (aux.color[0] * gD.double() * m).sum() \
            + (aux.color[1] * gA.double() * m).sum()
        ref = _grads_of(ref_loss, L)
        mf = m.float().to(dev)
        for v in hip_leaf.values():
            v.grad = None
        # (a map the loss does not look at is left out of it: the alpha-only backward is then handed no grad_depth and keeps
        # the segmented walk -- its segment-start term is what the windowed long-list case is there to check)
        loss = ((color * gC.to(dev)).sum(0) * mf).sum()
        if name in ("all", "depth"):
            loss = loss + (depth[0] * gD.to(dev) * mf).sum()
        if name in ("all", "alpha"):
            loss = loss + (alpha[0] * gA.to(dev) * mf).sum()
        loss.backward(retain_graph=True)
        torch.cuda.synchronize()
        line = []
        for k, gr in ref.items():
            gh = hip_leaf[k].grad
            if k in colour_names and name != "all":
                # the two maps reach no colour gradient: exactly zero, not merely small
                assert gh is None or float(gh.abs().max()) == 0.0, f"{tag}/{name}: {k} must be exactly zero"
                continue
            assert gh is not None, f"{tag}/{name}: no gradient for {k}"
            norm, frac = grad_error(gh, gr, elem_tol=5 * GRAD_TOL)
            line.append(f"{k} {norm:.1e}/{frac:.1e}")
            assert norm <= GRAD_TOL, f"{tag}/{name}: grad {k} normwise rel err {norm:.3e}"
            assert frac <= 1e-3, f"{tag}/{name}: grad {k}: {frac:.2e} of the significant elements off"
        if name != "all":
            ko = "opacities" if "opacities" in hip_leaf else "_opacity"
            assert float(hip_leaf[ko].grad.abs().max()) > 0.0
        print(f"[{tag}/{name}] grads (norm/frac): " + ", ".join(line))


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("bgv", [(0.0, 0.0, 0.0), (0.1, 0.7, 0.3)])
def test_parity_small_scene_classic_and_raw(view, bgv):
    D = _D()
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(n_views=2)
    cam, bg = cams[view], torch.tensor(bgv)
    inp = model_inputs(model, with_objs=False)
    st = settings_for(cam, bg)
    keys = hip_depth_keys(inp, cam, bg)
    H, W = cam.image_height, cam.image_width
    losses = _three_losses(H, W)
    with torch.no_grad():
        r32 = oracle_aux(inp, lambda L: L, st, keys, dtype=torch.float32)[:2]
    # classic surface
    col, aux, L, z_far = oracle_aux(inp, lambda L: L, st, keys)
    assert (aux.color[1].detach() - (1.0 - aux.final_T.detach())).abs().max().item() <= 1e-15
    fragile = col.fragile_px | aux.fragile_px
    share = fragile.float().mean().item()
    print(f"fragile share {share:.4f} (cap {FRAG_CAP})")
    assert share <= FRAG_CAP
    solid = ~fragile
    out, leaf = hip_classic(D, inp, cam, bg, dev)
    _compare(f"classic v{view}", out, leaf, col, aux, L, z_far, r32, losses, solid, dev, ("shs",))
    # raw surface: the oracle differentiates through the getters
    rawl = {k: getattr(model, k) for k in RAW}
    col, aux, L, z_far = oracle_aux(rawl, _act_raw, st, keys)
    out, leaf = hip_raw(D, model, cam, bg, dev)
    _compare(f"raw v{view}", out, leaf, col, aux, L, z_far, r32, losses, solid, dev, ("_features_dc", "_features_rest"))


def _raw_run(D, model, cam, bg, dev, aux, flags=0, g=None):
    out, leaf = hip_raw(D, model, cam, bg, dev, aux=aux, flags=flags)
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(3)
    gC, gD, gA = (torch.randn(3, H, W, generator=gen).to(dev), torch.randn(1, H, W, generator=gen).to(dev),
                  torch.randn(1, H, W, generator=gen).to(dev))
    if g is not None:
        gC, gD, gA = g
    loss = (out[0] * gC).sum()
    if aux:
        if gD is not None:
            loss = loss + (out[3] * gD).sum()
        if gA is not None:
            loss = loss + (out[4] * gA).sum()
    loss.backward()
    torch.cuda.synchronize()
    return out, {k: v.grad for k, v in leaf.items()}


def test_nothing_else_moves():
    """aux=True changes nothing else.  Absent aux gradients, or all-zero ones that leave the walk as it is (grad_alpha: the
    segmented walk stays), give the plain backward's bits.  An all-zero grad_depth makes the backward walk whole lists
    (the boundary records hold no running depth): bit for bit the plain backward under the same walk
    (GSR_FLAG_NO_SEGMENTS), and within the split / segment bound of tests/test_gpu_segments.py otherwise."""
    D = _D()
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(n_views=2)
    bg = torch.tensor([0.2, 0.1, 0.4])
    for cam in cams:
        H, W = cam.image_height, cam.image_width
        gC = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
        zero = torch.zeros(1, H, W, device=dev)
        for flags in (0, D.FLAG_NO_SEGMENTS):
            plain, gp = _raw_run(D, model, cam, bg, dev, aux=False, flags=flags, g=(gC, None, None))
            for tag, g in (("absent", (gC, None, None)), ("zero alpha", (gC, None, zero)), ("zero depth", (gC, zero, zero))):
                a, ga = _raw_run(D, model, cam, bg, dev, aux=True, flags=flags, g=g)
                assert torch.equal(a[0], plain[0]) and torch.equal(a[1], plain[1]) and torch.equal(a[2], plain[2])
                assert torch.equal(a[4][0], 1.0 - D.export_state(a[0], "final_T").view_as(a[4][0]))
                for k in gp:
                    if tag == "zero depth" and flags == 0:
                        assert _rel(ga[k], gp[k]) <= SPLIT_TOL, f"{k} moved by {_rel(ga[k], gp[k]):.2e} ({tag})"
                    else:
                        assert torch.equal(ga[k], gp[k]), f"{k} moved ({tag}, flags {flags:#x})"
        a1, g1 = _raw_run(D, model, cam, bg, dev, aux=True)
        a2, g2 = _raw_run(D, model, cam, bg, dev, aux=True)
        assert torch.equal(a1[3], a2[3]) and torch.equal(a1[4], a2[4])
        for k in g1:
            assert torch.equal(g1[k], g2[k]), f"{k}: two runs differ"


def _rel(a, b):
    s = b.abs().max().item()
    return (a - b).abs().max().item() / s if s > 0 else a.abs().max().item()


def _instantiation_sweep(model, cam, bg, configs, bitwise_names):
    D = _D()
    dev = torch.device("cuda:0")
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(11)
    g_all = (torch.randn(3, H, W, generator=gen).to(dev), torch.randn(1, H, W, generator=gen).to(dev),
             torch.randn(1, H, W, generator=gen).to(dev))
    z3 = torch.zeros_like(g_all[0])
    for lname, g in (("all", g_all), ("depth", (z3, g_all[1], None)), ("alpha", (z3, None, g_all[2]))):
        base, gb = _raw_run(D, model, cam, bg, dev, aux=True, g=g)
        for name, flags in configs:
            o, gg = _raw_run(D, model, cam, bg, dev, aux=True, flags=flags, g=g)
            assert torch.equal(o[3], base[3]) and torch.equal(o[4], base[4]) and torch.equal(o[0], base[0]), f"{name}: maps differ"
            for k in gb:
                if gb[k] is None:
                    continue
                if name in bitwise_names:
                    assert torch.equal(gg[k], gb[k]), f"{lname}/{name}: {k} not bit-identical"
                else:
                    r = _rel(gg[k], gb[k])
                    assert r <= SPLIT_TOL, f"{lname}/{name}: {k} differs by {r:.2e} of its largest gradient"


def test_every_instantiation_gives_the_same_maps():
    D = _D()
    model, cams, _ = _scene(n_views=2)
    cfg = [("fwd1", D.flag_fwd_split(1)), ("fwd2", D.flag_fwd_split(2)), ("fwd4", D.flag_fwd_split(4)),
           ("fwd1s", D.flag_fwd_split(1) | D.FLAG_FWD_SHARED), ("fwd2s", D.flag_fwd_split(2) | D.FLAG_FWD_SHARED),
           ("bwd2", D.flag_bwd_split(2)), ("bwd4", D.flag_bwd_split(4)),
           ("map0", D.flag_tile_map(0)), ("map1", D.flag_tile_map(1)), ("map2", D.flag_tile_map(2)), ("map3", D.flag_tile_map(3)),
           ("noseg", D.FLAG_NO_SEGMENTS), ("nocull", D.FLAG_NO_CULL), ("noside", D.FLAG_NO_SIDE_STREAM)]
    bitwise = {"fwd1", "fwd2", "fwd4", "fwd1s", "fwd2s", "map0", "map1", "map2", "map3", "noside"}
    _instantiation_sweep(model, cams[1], torch.tensor([0.3, 0.3, 0.1]), cfg, bitwise)


LONG = [("hydrant-full", dict(P=120000, width=480, height=400)), ("nyc-1M", dict(P=400000, width=960, height=544))]


@pytest.mark.parametrize("scene,kw", LONG)
def test_long_lists_segmented_walk_equals_whole_lists(scene, kw):
    """The two scenes of tests/test_gpu_segments.py: tiles are split into segments; the alpha-only backward walks segments,
    the depth backward whole lists; the three losses against GSR_FLAG_NO_SEGMENTS and the other backward split."""
    D = _D()
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(scene, device=dev, n_views=1, **kw)
    cam, bg = cams[0], torch.tensor([0.0, 0.0, 0.0])
    out, _ = hip_raw(D, model, cam, bg, dev)
    lens = D.export_state(out[0], "ranges").view(-1, 2).long()
    assert int(((lens[:, 1] - lens[:, 0]) > 256).sum()) > 5, "the scene must have split tiles"
    _instantiation_sweep(model, cam, bg, [("noseg", D.FLAG_NO_SEGMENTS), ("bwd2", D.flag_bwd_split(2)),
                                          ("bwd4 map0", D.flag_bwd_split(4) | D.flag_tile_map(0))], set())


WINDOW_FRAG_CAP = 0.08     # tests/test_gpu_fullsize_parity.py::compare, frag_frac: the cap of the windowed long-list comparisons


def test_long_lists_against_the_oracle_on_tile_windows():
    """S-hydrant-full (120 000 @ 480x400), eight single-tile windows whose lists are split in two or three segments (four
    tiles evenly spaced among those with 256 < len <= 512, four among 400 < len <= 800): maps and gradients of the three
    losses against oracle-R on those windows -- the segment-start term of the alpha channel, (T_b - T_final) g_A, against
    a reference that has no segments.  The oracle with its OWN depth order flags 0.011 / 0.012 of these windows' pixels
    fragile (CPU run), under the windowed comparisons' cap."""
    D = _D()
    dev = torch.device("cuda:0")
    kw = dict(P=120000, width=480, height=400)
    model, cams, _ = _scene("hydrant-full", device=dev, n_views=1, **kw)
    cpu_model, cpu_cams, _ = _scene("hydrant-full", n_views=1, **kw)
    cam, bg = cams[0], torch.tensor([0.0, 0.0, 0.0])
    H, W = cam.image_height, cam.image_width
    gx = (W + 15) // 16
    out, leaf = hip_raw(D, model, cam, bg, dev)
    assert D.export_state(out[0], "dv") is not None
    rg = D.export_state(out[0], "ranges").view(-1, 2).long().cpu()
    lens = rg[:, 1] - rg[:, 0]
    wins = []
    for lo, hi in ((256, 512), (400, 800)):
        idx = torch.nonzero((lens > lo) & (lens <= hi)).flatten()
        assert idx.numel() >= 4
        for t in idx[torch.linspace(0, idx.numel() - 1, 4).long()].tolist():
            wins.append((t % gx, t // gx, t % gx + 1, t // gx + 1))
    wins = sorted(set(wins))
    inp = model_inputs(cpu_model, with_objs=False)
    st = settings_for(cpu_cams[0], bg)
    keys = hip_depth_keys(inp, cpu_cams[0], bg)
    rawl = {k: getattr(cpu_model, k) for k in RAW}
    col, aux, L, z_far = oracle_aux(rawl, _act_raw, st, keys, tile_windows=wins)
    with torch.no_grad():
        r32 = oracle_aux(rawl, _act_raw, st, keys, dtype=torch.float32, tile_windows=wins)[:2]
    wpx = col.window_px
    fragile = (col.fragile_px | aux.fragile_px) & wpx
    share = fragile.sum().item() / wpx.sum().item()
    print(f"[windows] {len(wins)} tiles, lists {[int(lens[w[1] * gx + w[0]]) for w in wins]}, fragile share {share:.4f} (cap {WINDOW_FRAG_CAP})")
    assert share <= WINDOW_FRAG_CAP
    solid = wpx & ~fragile
    # (outside the windows the oracle's outputs are zero and the loss does not look: `solid` masks both sides)
    _compare("hydrant-full windows", out, leaf, col, aux, L, z_far, r32, _three_losses(H, W, seed=17), solid, dev,
             ("_features_dc", "_features_rest"), yard_mask=wpx)


@pytest.mark.parametrize("B", [1, 2, 5, 16])
def test_batch_equals_single_views(B):
    D = _D()
    from gsplat_attack import renderer as R
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(device=dev, n_views=B)
    from gsplat_attack.cameras import look_at_camera
    for v in range(1, B, 2):                           # per-view fields of view (x and y apart), per-view backgrounds below
        th = 2.0 * math.pi * v / B
        cams[v] = look_at_camera((2.0 * math.sin(th), -0.3, -2.0 * math.cos(th)), (0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0),
                                 fovx=0.55 + 0.03 * v, fovy=0.75 - 0.02 * v, width=cams[0].image_width,
                                 height=cams[0].image_height, uid=100 + v, device=dev)
    P = int(model.get_xyz.shape[0])
    pipe = R.PipelineParams(skip_objects=True)
    bgs = [torch.tensor([0.05 * v, 0.3, 1.0 - 0.05 * v], device=dev) for v in range(B)]
    H, W = cams[0].image_height, cams[0].image_width
    gen = torch.Generator().manual_seed(5)
    gC = torch.randn(B, 3, H, W, generator=gen).to(dev)
    gD = torch.randn(B, 1, H, W, generator=gen).to(dev)
    gA = torch.randn(B, 1, H, W, generator=gen).to(dev)
    sts = [R._settings(c, model, pipe, bgs[v], 1.0) for v, c in enumerate(cams)]
    # the loop: B single-view aux renders, gradients accumulated in a bucket in view order (gsr_backward_raw_into)
    loop = D.GradBucket(P, dev)
    exact = torch.zeros(59 * P, dtype=torch.float64, device=dev)
    own = D.GradBucket(P, dev)
    singles, vs = [], []
    for v in range(B):
        for bucket in (loop, own):
            if bucket is own:
                own.reset()
            m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
            o = D.rasterize_gaussians_raw(model._xyz, m2, model._features_dc, model._features_rest, None, model._opacity,
                                          model._scaling, model._rotation, sts[v], grad_bucket=bucket, aux=True)
            ((o[0] * gC[v]).sum() + (o[3] * gD[v]).sum() + (o[4] * gA[v]).sum()).backward()
        exact += own.flat.double()
        singles.append(o)
        vs.append(m2.grad)
    bat = D.GradBucket(P, dev)
    vsp = torch.zeros(B, P, 3, device=dev, requires_grad=True)
    image, radii, depth, alpha = D.rasterize_gaussians_raw_batch(model._xyz, vsp, model._features_dc, model._features_rest,
                                                                 model._opacity, model._scaling, model._rotation, sts,
                                                                 grad_bucket=bat, aux=True)
    ((image * gC).sum() + (depth * gD).sum() + (alpha * gA).sum()).backward()
    torch.cuda.synchronize()
    for v in range(B):
        assert torch.equal(image[v], singles[v][0]) and torch.equal(depth[v], singles[v][3]) and torch.equal(alpha[v], singles[v][4]), v
        assert torch.equal(vsp.grad[v], vs[v]), f"view {v}: screen-space gradient differs"
    bit_exact = os.environ.get("GSR_BATCH_K9", "1") == "0" or B == 1
    for name, s1, s2, c0, c1 in zip(loop.NAMES, loop.slices(), bat.slices(), loop.CUTS[:-1], loop.CUTS[1:]):
        if bit_exact:
            assert torch.equal(s1, s2), f"{name}: batched gradients differ from the accumulated single-view ones"
        else:                                          # the yardstick of tests/test_gpu_batch.py::_check_equal
            ex = exact[c0 * P:c1 * P]
            sc = ex.abs().max().item()
            e_seq, e_bat = (s1.double() - ex).abs().max().item(), (s2.double() - ex).abs().max().item()
            floor = 1e-4 if name in ("_scaling", "_rotation") else 1e-5
            assert e_bat <= max(3.0 * e_seq, floor * sc), f"{name}: batch {e_bat:.3e}, loop {e_seq:.3e}, scale {sc:.3e}"


def test_batch_against_the_oracle_sum():
    D = _D()
    from gsplat_attack import renderer as R
    dev = torch.device("cuda:0")
    B = 2
    model, cams, _ = _scene(device=dev, n_views=B)
    cpu_model, cpu_cams, _ = _scene(n_views=B)
    pipe = R.PipelineParams(skip_objects=True)
    bg = torch.tensor([0.0, 0.0, 0.0])
    H, W = cams[0].image_height, cams[0].image_width
    losses = _three_losses(H, W, seed=21)["all"]
    inp = model_inputs(cpu_model, with_objs=False)
    rawl = {k: getattr(cpu_model, k) for k in RAW}
    total, masks = None, []
    for v in range(B):
        st = settings_for(cpu_cams[v], bg)
        keys = hip_depth_keys(inp, cpu_cams[v], bg)
        col, aux, L, _ = oracle_aux(rawl, _act_raw, st, keys)
        m = (~(col.fragile_px | aux.fragile_px)).double()
        masks.append(m)
        loss = ((col.color * losses[0].double()).sum(0) * m).sum() + (aux.color[0] * losses[1].double() * m).sum() \
            + (aux.color[1] * losses[2].double() * m).sum()
        g = _grads_of(loss, L)
        total = g if total is None else {k: total[k] + g[k] for k in g if k != "means2D"}
    leaf = {k: getattr(model, k).detach().clone().requires_grad_(True) for k in RAW}
    sts = [R._settings(c, model, pipe, bg.to(dev), 1.0) for c in cams]
    image, radii, depth, alpha = D.rasterize_gaussians_raw_batch(leaf["_xyz"], None, leaf["_features_dc"], leaf["_features_rest"],
                                                                 leaf["_opacity"], leaf["_scaling"], leaf["_rotation"], sts, aux=True)
    mk = torch.stack(masks).float().to(dev)
    ((image * losses[0].to(dev)).sum(1) * mk).sum().add((depth[:, 0] * losses[1].to(dev) * mk).sum()).add(
        (alpha[:, 0] * losses[2].to(dev) * mk).sum()).backward()
    for k in RAW:
        norm, frac = grad_error(leaf[k].grad, total[k], elem_tol=5 * GRAD_TOL)
        print(f"[batch vs oracle sum] {k}: {norm:.2e} / {frac:.2e}")
        assert norm <= GRAD_TOL and frac <= 1e-3, k


def test_edges_empty_culled_ragged_twice_nograd():
    D = _D()
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(device=dev, n_views=1)
    cam = cams[0]
    bg = torch.tensor([0.3, 0.2, 0.1])
    st = settings_for(cam, bg, cls=D.GaussianRasterizationSettings, device=dev)
    H, W = cam.image_height, cam.image_width
    # empty scene: both maps all zero, no error, on both surfaces
    e = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    o = D.GaussianRasterizer(raster_settings=st)(means3D=e(0, 3), means2D=e(0, 3), opacities=e(0, 1), shs=e(0, 16, 3),
                                                 scales=e(0, 3), rotations=e(0, 4), aux=True)
    assert float(o[3].detach().abs().max()) == 0.0 and float(o[4].detach().abs().max()) == 0.0 and o[3].shape == (1, H, W)
    # (an empty scene has nothing to differentiate on either surface, with or without the maps)
    with torch.no_grad():
        o = D.rasterize_gaussians_raw(e(0, 3), e(0, 3), e(0, 1, 3), e(0, 15, 3), None, e(0, 1), e(0, 3), e(0, 4), st, aux=True)
    assert float(o[3].abs().max()) == 0.0 and float(o[4].abs().max()) == 0.0
    # everything culled: behind the camera
    leaf = {k: getattr(model, k).detach().clone().requires_grad_(True) for k in RAW}
    far = (leaf["_xyz"].detach() * 0.0 + cam.camera_center.to(dev)
           - 50.0 * cam.world_view_transform[:3, 2].to(dev)).requires_grad_(True)
    o = D.rasterize_gaussians_raw(far, torch.zeros_like(far), leaf["_features_dc"], leaf["_features_rest"], None, leaf["_opacity"],
                                  leaf["_scaling"], leaf["_rotation"], st, aux=True)
    assert int((o[1] > 0).sum()) == 0 and float(o[3].abs().max()) == 0.0 and float(o[4].abs().max()) == 0.0
    (o[3].sum() + o[4].sum()).backward()
    assert float(far.grad.abs().max()) == 0.0 and float(leaf["_opacity"].grad.abs().max()) == 0.0
    # ragged image smaller than a tile, against the single-flag sweep's own base run
    small, scams, _ = _scene(device=dev, n_views=1, width=13, height=9)
    a1, g1 = _raw_run(D, small, scams[0], bg, dev, aux=True)
    a2, g2 = _raw_run(D, small, scams[0], bg, dev, aux=True, flags=D.flag_fwd_split(4) | D.flag_bwd_split(4))
    assert a1[3].shape == (1, 9, 13) and torch.equal(a1[3], a2[3]) and torch.equal(a1[4], a2[4])
    assert torch.equal(a1[4][0], 1.0 - D.export_state(a1[0], "final_T").view(9, 13))
    # backward twice on one forward
    out, leaf = hip_raw(D, model, cam, bg, dev)
    loss = out[3].sum() * 0.5 + out[4].sum()
    loss.backward(retain_graph=True)
    first = {k: v.grad.clone() for k, v in leaf.items() if v.grad is not None}
    for v in leaf.values():
        v.grad = None
    loss.backward()
    for k, gfirst in first.items():
        assert torch.equal(leaf[k].grad, gfirst), k
    # no_grad keeps no context
    with torch.no_grad():
        o = D.rasterize_gaussians_raw(model._xyz, torch.zeros_like(model._xyz), model._features_dc, model._features_rest, None, model._opacity,
                                      model._scaling, model._rotation, st, aux=True)
    assert o[3].grad_fn is None and not o[3].requires_grad
    assert torch.equal(o[3], out[3]) and torch.equal(o[4], out[4])


def test_nonfinite_gaussians_leave_maps_and_gradients_alone():
    D = _D()
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(device=dev, n_views=1)
    cam, bg = cams[0], torch.tensor([0.0, 0.0, 0.0])
    clean, gclean = _raw_run(D, model, cam, bg, dev, aux=True)
    bad = copy.deepcopy(model)
    P = int(model.get_xyz.shape[0])
    idx = torch.arange(0, 40, device=dev)
    # appended (not replaced) Gaussians, broken in turn: NaN / inf in mean, scale, rotation
    def grow(t, fill):
        extra = t.detach()[idx].clone()
        fill(extra)
        return torch.nn.Parameter(torch.cat([t.detach(), extra]))
    nan, inf = float("nan"), float("inf")
    bad._xyz = grow(model._xyz, lambda x: (x[:10].fill_(nan), x[10:20, 0].fill_(inf)))
    bad._scaling = grow(model._scaling, lambda x: x[20:30].fill_(inf))
    bad._rotation = grow(model._rotation, lambda x: x[30:40].fill_(nan))
    for name in ("_features_dc", "_features_rest", "_opacity"):
        setattr(bad, name, grow(getattr(model, name), lambda x: None))
    out, g = _raw_run(D, bad, cam, bg, dev, aux=True)
    assert torch.equal(out[3], clean[3]) and torch.equal(out[4], clean[4]) and torch.equal(out[0], clean[0])
    for k in RAW:
        assert torch.equal(g[k][:P], gclean[k]), k
        assert float(g[k][P:].abs().max()) == 0.0, f"{k}: a culled Gaussian received a gradient"


def test_refusals_are_errors_with_messages_never_silent():
    D = _D()
    import ctypes
    from gsplat_attack import renderer as R
    dev = torch.device("cuda:0")
    lib = D._load()
    model, cams, _ = _scene(device=dev, n_views=2)
    bg = torch.tensor([0.0, 0.0, 0.0], device=dev)
    pipe = R.PipelineParams(skip_objects=True)
    H, W = cams[0].image_height, cams[0].image_width
    P = int(model.get_xyz.shape[0])
    gd = torch.ones(2, H, W, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    # a context whose forward produced no maps cannot be armed
    plain = R.render(cams[0], model, pipe, bg)
    h = plain["render"].grad_fn.holder.handle
    assert lib.gsr_ctx_set_aux_grads(h, ptr(gd), None) == 4          # GSR_ERR_STATE
    assert b"did not produce" in lib.gsr_last_error()
    # per-view batch backward with an armed context: refused, and the request does not survive the refusal
    sts = [R._settings(c, model, pipe, bg, 1.0) for c in cams]
    vsp = torch.zeros(2, P, 3, device=dev, requires_grad=True)
    bset = D.GradBucketSet(2, P, dev)
    image, radii, depth, alpha = D.rasterize_gaussians_raw_batch(model._xyz, vsp, model._features_dc, model._features_rest,
                                                                 model._opacity, model._scaling, model._rotation, sts,
                                                                 grad_bucket=bset, aux=True)
    with pytest.raises(RuntimeError, match="per-view"):
        (image.sum() + depth.sum()).backward()
    # the chunked backward
    bucket = D.GradBucket(P, dev)
    bucket.chunks = 4
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    o = D.rasterize_gaussians_raw(model._xyz, m2, model._features_dc, model._features_rest, None, model._opacity,
                                  model._scaling, model._rotation, sts[0], grad_bucket=bucket, aux=True)
    with pytest.raises(RuntimeError, match="chunked"):
        (o[0].sum() + o[4].sum()).backward()
    # aux gradients together with grad_objects
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    obj = torch.randn(P, 1, 16, device=dev, requires_grad=True)
    o = D.rasterize_gaussians_raw(model._xyz, m2, model._features_dc, model._features_rest, obj, model._opacity,
                                  model._scaling, model._rotation, sts[0], aux=True)
    with pytest.raises(RuntimeError, match="grad_objects"):
        (o[2].sum() + o[3].sum()).backward()
    # ... but the object map with aux outputs and no dL/dobjects works
    o = D.rasterize_gaussians_raw(model._xyz, m2, model._features_dc, model._features_rest, obj, model._opacity,
                                  model._scaling, model._rotation, sts[0], aux=True)
    (o[0].sum() + o[3].sum()).backward()
    # GSR_FLAG_NEEDLE_DOUBLE, objects in an aux batch, an aux render through a RenderCache (bypassed: no hit, right maps)
    with D.extra_flags(D.FLAG_NEEDLE_DOUBLE):
        with pytest.raises(Exception, match="NEEDLE_DOUBLE"):
            D.rasterize_gaussians_raw(model._xyz, m2, model._features_dc, model._features_rest, None, model._opacity,
                                      model._scaling, model._rotation, sts[0], aux=True)
    with pytest.raises(ValueError, match="objects_dc"):
        D.rasterize_gaussians_raw_batch(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                        model._scaling, model._rotation, sts, objects_dc=obj, aux=True)
    cache = D.RenderCache()
    pc = R.PipelineParams(skip_objects=True, render_cache=cache, aux_outputs=True)
    with torch.no_grad():
        r1 = R.render(cams[0], model, pc, bg)
        r2 = R.render(cams[0], model, pc, bg)
    assert cache.hits == 0 and torch.equal(r1["render_alpha"], r2["render_alpha"]) and torch.equal(r1["render_depth"], r2["render_depth"])


def test_consumers_render_keys_composite_over_and_alpha_boxes():
    D = _D()
    from gsplat_attack import renderer as R
    from gsplat_attack import composite_over, benign_bboxes
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(device=dev, n_views=2)
    cpu_model, cpu_cams, _ = _scene(n_views=2)
    black = torch.zeros(3, device=dev)
    today = {"render", "viewspace_points", "visibility_filter", "radii", "render_object"}
    for fused in (True, False):
        plain = R.render(cams[0], model, R.PipelineParams(fused_activations=fused), black)
        assert set(plain.keys()) == today
        res = R.render(cams[0], model, R.PipelineParams(fused_activations=fused, aux_outputs=True), black)
        assert set(res.keys()) == today | {"render_depth", "render_alpha"}
        assert torch.equal(res["render"], plain["render"]) and res["render_alpha"].shape == (1,) + tuple(plain["render"].shape[1:])
    assert set(R.render_batch(cams, model, R.PipelineParams(skip_objects=True), black).keys()) == today
    rb = R.render_batch(cams, model, R.PipelineParams(skip_objects=True, aux_outputs=True), black)
    assert set(rb.keys()) == today | {"render_depth", "render_alpha"} and rb["render_alpha"].shape[:2] == (2, 1)
    # composite_over a photo-like background: the oracle renders on black and pastes in float64
    cam, ccam = cams[0], cpu_cams[0]
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(13)
    photo = torch.rand(3, H, W, generator=gen)
    gL = torch.randn(3, H, W, generator=gen)
    inp = model_inputs(cpu_model, with_objs=False)
    st = settings_for(ccam, torch.zeros(3))
    keys = hip_depth_keys(inp, ccam, torch.zeros(3))
    rawl = {k: getattr(cpu_model, k) for k in RAW}
    col, aux, L, _ = oracle_aux(rawl, _act_raw, st, keys)
    fragile = col.fragile_px | aux.fragile_px
    m = (~fragile).double()
    ref = col.color + (1.0 - aux.color[1]) * photo.double()
    gref = _grads_of(((ref * gL.double()).sum(0) * m).sum(), L)["_opacity"]
    res = R.render(cam, model, R.PipelineParams(skip_objects=True, aux_outputs=True), black)
    pasted = composite_over(res, photo.to(dev))
    err = (pasted.detach().cpu().double() - ref.detach()).abs().amax(0)[~fragile].max().item()
    print(f"composite_over: solid err {err:.2e}")
    assert err <= 1e-4
    model._opacity.grad = None
    ((pasted * gL.to(dev)).sum(0) * m.float().to(dev)).sum().backward()
    norm, frac = grad_error(model._opacity.grad, gref, elem_tol=5 * GRAD_TOL)
    print(f"composite_over: dL/d_opacity {norm:.2e} / {frac:.2e}")
    assert norm <= 1e-3
    both = composite_over(rb, photo.to(dev))
    assert both.shape == rb["render"].shape and torch.equal(both[0], pasted.detach())
    with pytest.raises(ValueError, match="black"):
        composite_over(R.render(cam, model, R.PipelineParams(skip_objects=True, aux_outputs=True),
                                torch.tensor([0.5, 0.5, 0.5], device=dev)), photo.to(dev))
    # alpha boxes: getbbox of the oracle's alpha map, up to fragile pixels on the box's edge rows / columns
    boxes = benign_bboxes(model, cams[:1], alpha_threshold=0.5)
    on = aux.color[1].detach() > 0.5
    sure = on & ~fragile
    maybe = on | fragile
    rows, cols = torch.nonzero(sure.any(1)).flatten(), torch.nonzero(sure.any(0)).flatten()
    rows_m, cols_m = torch.nonzero(maybe.any(1)).flatten(), torch.nonzero(maybe.any(0)).flatten()
    l, u, r, d = boxes[0]
    assert int(cols_m[0]) <= l <= int(cols[0]) and int(rows_m[0]) <= u <= int(rows[0])
    assert int(cols[-1]) + 1 <= r <= int(cols_m[-1]) + 1 and int(rows[-1]) + 1 <= d <= int(rows_m[-1]) + 1
    exact = (int(torch.nonzero(on.any(0)).flatten()[0]), int(torch.nonzero(on.any(1)).flatten()[0]),
             int(torch.nonzero(on.any(0)).flatten()[-1]) + 1, int(torch.nonzero(on.any(1)).flatten()[-1]) + 1)
    print("alpha box", boxes[0], "oracle", exact)
    assert benign_bboxes(model, cams[:1]) == [__import__("gsplat_attack.attack", fromlist=["x"]).bbox_from_render(
        R.render(cam, model, R.PipelineParams(skip_objects=True), black)["render"])]


def test_object_channels_with_maps_every_forward_form():
    """The five forward forms with object channels AND the maps (k_render_fwd<true, NPX, WPB, true>): depth and alpha bit for
    bit those of the run without object features, colour and object map bit for bit those of aux=False."""
    D = _D()
    dev = torch.device("cuda:0")
    for scene, kw in (("hydrant-1k", {}), ("hydrant-full", dict(P=60000, width=480, height=400))):
        model, cams, _ = _scene(scene, device=dev, n_views=2, **kw)
        cam = cams[1]
        st = settings_for(cam, torch.tensor([0.3, 0.1, 0.2]), cls=D.GaussianRasterizationSettings, device=dev)
        P = int(model._xyz.shape[0])
        obj = torch.randn(P, 1, 16, generator=torch.Generator().manual_seed(4)).to(dev)

        def run(o, aux):
            with torch.no_grad():
                return D.rasterize_gaussians_raw(model._xyz, torch.zeros(P, 3, device=dev), model._features_dc,
                                                 model._features_rest, o, model._opacity, model._scaling, model._rotation,
                                                 st, aux=aux)
        for name, flags in (("default", 0), ("fwd1", D.flag_fwd_split(1)), ("fwd2", D.flag_fwd_split(2)),
                            ("fwd4", D.flag_fwd_split(4)), ("fwd1 shared", D.flag_fwd_split(1) | D.FLAG_FWD_SHARED),
                            ("fwd2 shared", D.flag_fwd_split(2) | D.FLAG_FWD_SHARED)):
            with D.extra_flags(flags):
                no_obj, plain, both = run(None, True), run(obj, False), run(obj, True)
            assert float(plain[2].abs().max()) > 0.0
            assert torch.equal(both[3], no_obj[3]) and torch.equal(both[4], no_obj[4]), f"{scene}/{name}: maps differ with object channels"
            assert torch.equal(both[0], plain[0]) and torch.equal(both[2], plain[2]) and torch.equal(both[1], plain[1]), \
                f"{scene}/{name}: colour / object map / radii differ with the maps"


def _closed(D, dev, xyz, scale, opac, K=16):
    """The camera of tests/test_gpu_closed_form.py (identity view, tan(fov / 2) = 1, 32 x 32: focal 16, centre (15.5, 15.5))."""
    from test_gpu_closed_form import _closed_form_settings
    n = len(xyz)
    means = torch.tensor(xyz, dtype=torch.float32, device=dev, requires_grad=True)
    sh = torch.zeros(n, K, 3, device=dev)               # (colour 0.5; 16 coefficients: the layout that takes the lane-group K9)
    op = torch.tensor(opac, dtype=torch.float32, device=dev).view(n, 1).requires_grad_(True)
    sc = torch.tensor([[s, s, s] for s in scale], dtype=torch.float32, device=dev)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * n, dtype=torch.float32, device=dev)
    st = _closed_form_settings(D, dev, [0.1, 0.2, 0.3])
    out = D.GaussianRasterizer(raster_settings=st)(means3D=means, means2D=torch.zeros(n, 3, device=dev), opacities=op, shs=sh,
                                                   scales=sc, rotations=rot, aux=True)
    return out, means, op


def _grads_at_centre(t, means, op):
    gm, go = torch.autograd.grad(t[0, 15, 15], [means, op], retain_graph=True)
    return gm.cpu().double(), go.flatten().cpu().double()


# Closed forms.  Footprint as derived in tests/test_gpu_closed_form.py: sigma^2 = (16 s / z)^2 + 0.3 = 4.3 for (s, z) = (0.5, 4)
# and (1, 8); pixel (15, 15) is (0.5, 0.5) from the centre: G = exp(-0.25 / 4.3) = 0.943518284537.  With x = y = 0 the centre
# does not move with z and the off-diagonal Jacobian terms and their z-derivatives vanish, so alpha depends on mean_z through
# sigma^2 alone: d sigma^2 / dz = -2 (16 s)^2 / z^3 (-2 for the front splat, -1 for the back one) and
# d alpha / d sigma^2 = alpha (r^2 / 2) / sigma^4 = alpha * 0.25 / 18.49.  Tolerances: the 2e-6 of the colour literals there,
# times the depth (<= 8) where a value is scaled by z.
CF_TOL = 2e-6
G_ = 0.943518284537107
K_ = 0.25 / 18.49


def test_closed_form_one_gaussian_depth_and_alpha():
    D = _D()
    dev = torch.device("cuda:0")
    (color, radii, _, depth, alpha), means, op = _closed(D, dev, [[0.0, 0.0, 4.0]], [0.5], [0.6])
    a1 = 0.566110970722264                                  # 0.6 G
    assert abs(alpha[0, 15, 15].item() - a1) <= CF_TOL
    assert abs(depth[0, 15, 15].item() - 2.264443882889056) <= 4 * CF_TOL          # z a1
    gm, go = _grads_at_centre(alpha, means, op)
    assert abs(go[0].item() - G_) <= CF_TOL                                     # dA/do = G
    assert abs(gm[0, 2].item() - (-0.015308571409472)) <= CF_TOL               # dA/dz = a1 K (-2)
    gm, go = _grads_at_centre(depth, means, op)
    assert abs(go[0].item() - 3.774073138148428) <= 4 * CF_TOL                 # dD/do = z G
    # dD/dmean_z = a1 (through z itself: dz/dmean_z = viewmatrix[2][2] = 1) + z dA/dz = 0.566110970722 - 0.061234285638
    assert abs(gm[0, 2].item() - 0.504876685084377) <= 4 * CF_TOL
    # dD/dX = z dA/dX,  dA/dX = -a1 (0.5 / 4.3) dpx/dX with dpx/dX = 16 / z = 4:  4 * (-0.263307421660)
    assert abs(gm[0, 0].item() - (-1.053229686641)) <= 4 * CF_TOL and abs(gm[0, 1].item() - (-1.053229686641)) <= 4 * CF_TOL


def test_closed_form_two_overlapping_gaussians_depth_and_alpha():
    """Back splat (z = 8, s = 1, o = 0.5) stored FIRST, front splat (z = 4, s = 0.5, o = 0.6): a2 = 0.5 G, a1 = 0.6 G,
    A = a1 + a2 (1 - a1), D = 4 a1 + 8 a2 (1 - a1)."""
    D = _D()
    dev = torch.device("cuda:0")
    (color, radii, _, depth, alpha), means, op = _closed(D, dev, [[0.0, 0.0, 8.0], [0.0, 0.0, 4.0]], [1.0, 0.5], [0.5, 0.6])
    a1, a2 = 0.566110970722264, 0.471759142268554
    assert abs(alpha[0, 15, 15].item() - 0.770802087014064) <= CF_TOL
    assert abs(depth[0, 15, 15].item() - 3.901972813223456) <= 8 * CF_TOL
    gm, go = _grads_at_centre(alpha, means, op)
    assert abs(go[0].item() - G_ * (1 - a1)) <= CF_TOL and abs(go[1].item() - G_ * (1 - a2)) <= CF_TOL
    assert abs(gm[0, 2].item() - (-a2 * K_ * (1 - a1))) <= CF_TOL                # -0.002767592162
    assert abs(gm[1, 2].item() - (-2 * a1 * K_ * (1 - a2))) <= CF_TOL            # -0.008086612892
    gm, go = _grads_at_centre(depth, means, op)
    assert abs(go[0].item() - 3.275057860668799) <= 8 * CF_TOL                    # 8 G (1 - a1)
    assert abs(go[1].item() - 0.213166125125047) <= 8 * CF_TOL                    # G (4 - 8 a2)
    # back: a2 (1 - a1) through z, + 8 (1 - a1) dalpha2/dz;  front: a1 through z, + (4 - 8 a2) dalpha1/dz
    assert abs(gm[0, 2].item() - 0.182550378996851) <= 8 * CF_TOL
    assert abs(gm[1, 2].item() - 0.562652353224292) <= 8 * CF_TOL


def test_colour_only_attack_through_composite_over_and_rerender_refusal():
    """Only the colour parameters require a gradient and the screen-space gradient is off: the maps' gradients reach nothing
    that is wanted, are not handed to the library, and the colour gradients are those of the plain render.  And a context
    with maps is not re-rendered: gsr_ctx_rerender returns GSR_ERR_STATE before it launches anything."""
    D = _D()
    import ctypes
    from gsplat_attack import renderer as R
    from gsplat_attack import composite_over
    dev = torch.device("cuda:0")
    model, cams, _ = _scene(device=dev, n_views=1)
    for k in ("_xyz", "_opacity", "_scaling", "_rotation"):
        getattr(model, k).requires_grad_(False)
    cam, black = cams[0], torch.zeros(3, device=dev)
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(2)
    photo, g = torch.rand(3, H, W, generator=gen).to(dev), torch.randn(3, H, W, generator=gen).to(dev)
    model.zero_grad()
    (R.render(cam, model, R.PipelineParams(skip_objects=True, viewspace_grad=False), black)["render"] * g).sum().backward()
    want = (model._features_dc.grad.clone(), model._features_rest.grad.clone())
    model.zero_grad()
    res = R.render(cam, model, R.PipelineParams(skip_objects=True, viewspace_grad=False, aux_outputs=True), black)
    (composite_over(res, photo) * g).sum().backward()
    assert torch.equal(model._features_dc.grad, want[0]) and torch.equal(model._features_rest.grad, want[1])
    lib = D._load()
    h = res["render"].grad_fn.holder.handle
    dst = torch.empty(3, H, W, device=dev)
    rc = lib.gsr_ctx_rerender(h, None, ctypes.c_void_p(model._features_rest.data_ptr()), None, None, None,
                              ctypes.c_void_p(dst.data_ptr()), None, 0, None)
    assert rc == 4 and b"not re-rendered" in lib.gsr_last_error()


def test_armed_classic_context_with_other_than_sixteen_coefficients_refuses():
    D = _D()
    dev = torch.device("cuda:0")
    (color, radii, _, depth, alpha), means, op = _closed(D, dev, [[0.0, 0.0, 4.0]], [0.5], [0.6], K=1)
    assert abs(alpha[0, 15, 15].item() - 0.566110970722264) <= CF_TOL          # the forward serves any K
    with pytest.raises(RuntimeError, match="K != 16"):
        depth[0, 15, 15].backward()
    color[0, 15, 15].backward()                         # the refused request is gone: a plain backward runs

"""The compositors (k_render_fwd / k_render_bwd) and the footprint cull (k_emit's strip masks, which the compositors do not
re-check) at the image's far edges, against oracle-R in float64 on ALL pixels and ALL Gaussians.  tests/far_edge_scenes.py
builds, for images that leave 1 .. 9 live columns / rows in the last tiles, for images smaller than a tile or one pixel
thin and for the two images of 65520 px, entries that sit in the last live pixels, reach them from beyond the edge, reach
only the corner pixel, or miss the image by a pixel (and must be culled); tests/test_far_edges_cpu.py holds the designed
facts to oracle-R with nothing fragile, so nothing is excused here.  Every case goes through run_single -> check_forward ->
check_grads of tests/test_gpu_list_edges.py with that module's bounds."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import far_edge_scenes as F
import list_edge_scenes as S
from test_gpu_list_edges import (FORM_NAMES, _D, _forms, batch_case, check_forward, check_grads, refs_for, run_single, seg_shift)

pytestmark = pytest.mark.gpu

GEOMETRY_FORMS = ["default-raw", "fwd1-classic-obj", "fwd2-raw-alpha", "fwd4-raw", "fwd1-shared-classic", "fwd2-shared-raw-obj",
                  "bwd2-classic-depth", "bwd4-raw-alpha"]
OTHER = tuple(k for k in F.SIZES if k not in F.CORE) + F.SMALL
CASES = [(k, f) for k in F.CORE for f in FORM_NAMES] + [(k, f) for k in OTHER for f in GEOMETRY_FORMS]


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for name, d in w.items():
        print(f"\n[far edges] {name}: worst errors against the float64 oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(d.items())))


def _case(sc, form, worst, r64=None, r32=None, view_of=lambda t: t):
    """One form on view 0 of a single-view scene, through the list-edge checks.  view_of: what of an image is compared."""
    D = _D()
    dev = torch.device("cuda:0")
    flags, surface, obj, aux, terms = _forms(D)[form]
    tw = getattr(sc, "tile_windows", None)                # (only the two scenes of 65520 px carry windows)
    res, grads = run_single(D, sc, flags, surface, obj, aux, terms, dev, tile_windows=tw)
    full = dict(res)
    res = {k: (view_of(v) if torch.is_tensor(v) else v) for k, v in res.items()}
    r64 = S.oracle_run(sc, 0, tile_windows=tw) if r64 is None else r64
    r32 = S.oracle_run(sc, 0, torch.float32, tile_windows=tw) if r32 is None else r32
    tag = f"{sc.name} / {form}"
    w = worst.setdefault(sc.name, {})
    check_forward(tag, sc, 0, res, r64, r32, bool(flags & D.FLAG_NO_SEGMENTS), w)
    ref64, ref32 = refs_for(sc, 0, terms, list(grads), tile_windows=tw)
    check_grads(tag, grads, ref64, ref32, S.dead_gaussians(sc), F.first_blended(sc.facts[0]), w)
    return full, grads


@pytest.mark.parametrize("key,form", CASES, ids=[f"{F.name_of(k)}-{f}" for k, f in CASES])
def test_far_edge_scenes_against_the_float64_oracle(key, form, worst):
    """All 21 forms on the three core sizes; on the other sizes the forms that change the wave geometry."""
    sc = F.get(key)
    assert S.dead_gaussians(sc).sum() >= sc.designed_drops > 0
    _case(sc, form, worst)


@pytest.mark.parametrize("key", F.SIZES + F.SMALL, ids=F.name_of)
def test_list_lengths_with_and_without_the_footprint_cull(key):
    """FLAG_NO_CULL keeps the miss and dead-strip pairs (the whole lists, n_contrib as the oracle numbers it); the default
    cull drops exactly the designed ones."""
    D = _D()
    dev = torch.device("cuda:0")
    sc = F.get(key)
    f = sc.facts[0]
    res, _ = run_single(D, sc, D.FLAG_NO_CULL, "raw", False, False, "C", dev)
    assert np.array_equal(res["lens"].reshape(f.tile_len.shape), f.tile_len)
    assert res["records"] == S.records(f.tile_len, seg_shift())
    assert torch.equal(res["n_contrib"], S.oracle_run(sc, 0).n_contrib)
    cull, _ = run_single(D, sc, 0, "raw", False, False, "C", dev)
    dropped = res["lens"].reshape(f.tile_len.shape) - cull["lens"].reshape(f.tile_len.shape)
    own = sum(int(dropped[ty, tx]) for tx, ty in sc.far_tiles)
    print(f"[far edges] {sc.name}: the cull dropped {int(dropped.sum())} pairs, designed {int((f.tile_len - f.tile_len_cull).sum())}; "
          f"{own} in the far-edge tiles, of which their own miss / dead-strip entries {sc.designed_drops}")
    assert np.array_equal(dropped, f.tile_len - f.tile_len_cull) and own >= sc.designed_drops
    assert torch.equal(cull["n_contrib"], res["n_contrib"]) and torch.equal(cull["color"], res["color"])


@pytest.mark.parametrize("key", F.CORE, ids=F.name_of)
def test_every_forward_instantiation_gives_the_same_bits(key):
    """Colour, final_T and n_contrib bit-identical across the forward splits, the shared-staging forms and the tile maps."""
    D = _D()
    dev = torch.device("cuda:0")
    sc = F.get(key)
    base, _ = run_single(D, sc, 0, "raw", False, False, "C", dev)
    for name, flags in (("fwd1", D.flag_fwd_split(1)), ("fwd2", D.flag_fwd_split(2)), ("fwd4", D.flag_fwd_split(4)),
                        ("fwd1s", D.flag_fwd_split(1) | D.FLAG_FWD_SHARED), ("fwd2s", D.flag_fwd_split(2) | D.FLAG_FWD_SHARED),
                        ("map0", D.flag_tile_map(0)), ("map1", D.flag_tile_map(1)), ("map2", D.flag_tile_map(2)),
                        ("map3", D.flag_tile_map(3))):
        res, _ = run_single(D, sc, flags, "raw", False, False, "C", dev)
        for k in ("color", "final_T", "n_contrib"):
            assert torch.equal(res[k], base[k]), f"{sc.name} / {name}: {k} differs from the default form's"


def _oracle_on_kept_lists(sc, v):
    """oracle-R's result with n_contrib numbered along the kept lists (far_edge_scenes.kept_numbering)."""
    r = S.oracle_run(sc, v)
    return SimpleNamespace(**{**vars(r), "n_contrib": torch.from_numpy(F.kept_numbering(sc.facts[v], r.n_contrib.numpy()))})


BATCH_CASES = [("default", "into"), ("fwd2-shared", "into"), ("bwd2", "into"), ("objects", "into"), ("default", "views"),
               ("bwd2", "views"), ("objects", "views")]


@pytest.mark.parametrize("form,mode", BATCH_CASES, ids=[f"{f}-{m}" for f, m in BATCH_CASES])
def test_batch_of_three_views_across_the_far_edge(form, mode, worst):
    """33 x 17, B = 3: the far-edge entries as built, moved inside the image, and moved across the near edges."""
    D = _D()
    dev = torch.device("cuda:0")
    sc = F.get(("batch", 3))
    out, leaf, vsp, bset = batch_case(sc, 3, form, mode, worst.setdefault(sc.name, {}), oracle=_oracle_on_kept_lists,
                                      first=F.first_blended)
    # every view bit-equal to its single-view render (and, view by view, to its single-view backward).  Not compared: the
    # gradient of _objects_dc, which the batch hands back as ONE tensor summed over the views, in no fixed association
    # with the single-view calls' sum (it is held to the float64 sum in batch_case).
    obj = form == "objects"
    flags = {"default": 0, "fwd2-shared": D.flag_fwd_split(2) | D.FLAG_FWD_SHARED, "bwd2": D.flag_bwd_split(2), "objects": 0}[form]
    nc = D.export_state(out[0], "n_contrib").view(3, sc.H, sc.W)
    fT = D.export_state(out[0], "final_T").view(3, sc.H, sc.W)
    for v, cam in enumerate(sc.cams):
        st = S.settings(cam, torch.tensor(S.BG), D.GaussianRasterizationSettings, device=dev)
        one = D.GradBucket(sc.P, dev)
        lf = {k: t.to(dev).clone().requires_grad_(obj or k != "_objects_dc") for k, t in sc.raw.items()}
        m2d = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
        with D.extra_flags(flags):
            o = D.rasterize_gaussians_raw(lf["_xyz"], m2d, lf["_features_dc"], lf["_features_rest"], lf["_objects_dc"] if obj else None,
                                          lf["_opacity"], lf["_scaling"], lf["_rotation"], st, grad_bucket=one)
            w = S.loss_weights(sc, v)
            loss = (o[0] * w["C"].to(dev)).sum()
            if obj:
                loss = loss + (o[2] * w["O"].to(dev)).sum()
            loss.backward()
            torch.cuda.synchronize()
        assert torch.equal(out[0][v].detach(), o[0].detach()), f"view {v}: the batched image differs from the single-view render"
        if obj:
            assert torch.equal(out[2][v].detach(), o[2].detach()), f"view {v}: the batched object map differs from the single-view render"
        assert torch.equal(nc[v], D.export_state(o[0], "n_contrib").view(sc.H, sc.W)), f"view {v}: n_contrib"
        assert torch.equal(fT[v], D.export_state(o[0], "final_T").view(sc.H, sc.W)), f"view {v}: final_T"
        assert torch.equal(vsp.grad[v], m2d.grad), f"view {v}: screen-space gradient"
        if mode == "views":
            assert torch.equal(bset.bucket(v).flat, one.flat), f"view {v}: gradients differ from the single-view backward"


@pytest.mark.parametrize("form", ["default-raw", "fwd2-shared-raw-obj", "bwd4-raw-alpha"])
def test_results_do_not_depend_on_what_the_workspace_pool_held(form, worst):
    """A core case, a larger unrelated scene (hydrant-1k at 320 x 192), the core case again: bit-equal outputs and gradients."""
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    dev = torch.device("cuda:0")
    sc = F.get((33, 17))
    a, ga = _case(sc, form, worst)
    model, cams, _ = make_scene("hydrant-1k", device=dev, n_views=1, width=320, height=192)
    out = render(cams[0], model, PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device=dev))
    out["render"].sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["render"]).all())
    b, gb = _case(sc, form, worst)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), f"{form}: {k} changed after an unrelated larger render"
        else:
            assert np.array_equal(a[k], b[k]), k
    for k in ga:
        assert (ga[k] is None and gb[k] is None) or torch.equal(ga[k], gb[k]), f"{form}: grad {k} changed after an unrelated larger render"


@pytest.mark.parametrize("form", ["default-raw", "fwd4-raw", "bwd4-raw-alpha"])
@pytest.mark.parametrize("horizontal", [True, False], ids=["65520x17", "17x65520"])
def test_the_largest_image_on_tile_windows(horizontal, form, worst):
    """65520 x 17 and 17 x 65520 (4095 tiles and a one-pixel remainder): colour, final_T, n_contrib and the gradients against
    oracle-R on tile windows around the first, the middle and the last tile of the long axis, dL/dC zero outside them;
    outside every Gaussian's tile rect the image is the background bit for bit.
    check_grads counts an element as off only beyond twice the float32 oracle's own error, and that oracle, which forms the
    pixel centre in image coordinates, is 2e-3 .. 5e-3 off here (tests/test_far_edges_cpu.py): `frac == 0` says little in
    these cases, and the normwise GRAD_TOL is the bound that bites (the device is about 1e-6 off)."""
    sc = F.get(("big", horizontal))
    crop = lambda t: F.crop(sc, t)
    r = {dt: S.oracle_run(sc, 0, dt, tile_windows=sc.tile_windows) for dt in (torch.float64, torch.float32)}
    rw = {dt: SimpleNamespace(**{k: (crop(v) if k in ("color", "objects", "depth", "alpha", "final_T", "n_contrib") else v)
                                 for k, v in vars(x).items()}) for dt, x in r.items()}
    full, _ = _case(sc, form, worst, rw[torch.float64], rw[torch.float32], view_of=lambda t: crop(t) if t.dim() >= 2 else t)
    empty = torch.from_numpy(np.kron(sc.facts[0].tile_len == 0, np.ones((16, 16), dtype=bool))[:sc.H, :sc.W])
    assert int(empty.sum()) > 0.99 * sc.H * sc.W
    bg = torch.tensor(S.BG)[:, None].expand(3, int(empty.sum()))
    assert torch.equal(full["color"][:, empty], bg), "a pixel outside every tile rect is not the background"
    assert int(full["n_contrib"][empty].abs().max()) == 0 and bool((full["final_T"][empty] == 1.0).all())


@pytest.mark.parametrize("entry", ["classic-width", "classic-height", "batch-width"])
def test_one_pixel_more_than_65520_is_refused(entry, worst):
    D = _D()
    dev = torch.device("cuda:0")
    sc = F.get((1, 1))
    W, H = (16, 65521) if entry == "classic-height" else (65521, 16)
    st = S.settings(S.camera(H, W, focal=F.BIG_FOCAL), torch.tensor(S.BG), D.GaussianRasterizationSettings, device=dev)
    raw = {k: v.to(dev) for k, v in sc.raw.items()}
    with pytest.raises(Exception, match="image larger than 65520 px per side"):
        if entry == "batch-width":
            D.rasterize_gaussians_raw_batch(raw["_xyz"], None, raw["_features_dc"], raw["_features_rest"], raw["_opacity"],
                                            raw["_scaling"], raw["_rotation"], [st, st])
        else:
            act = S.activate(raw)
            D.GaussianRasterizer(raster_settings=st)(means3D=act["means3D"], means2D=torch.zeros(sc.P, 3, device=dev),
                                                     opacities=act["opacities"], shs=act["shs"], scales=act["scales"],
                                                     rotations=act["rotations"])
    _case(F.get((16, 16)), "default-raw", worst)           # and the device still renders a tile rightly

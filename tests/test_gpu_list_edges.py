"""The compositors (k_render_fwd / k_render_bwd) on the list-length and stop-index edges, against oracle-R in float64 on
ALL pixels and ALL Gaussians: tests/list_edge_scenes.py builds scenes whose lists are exactly 63 / 64 / 65 ... 1025 entries
long and whose pixels stop at designed entries, with no fragile pixel (tests/test_list_edges_cpu.py), so nothing is excused.

Per scene and form: list lengths and the boundary-record count against the DESIGNED lengths; n_contrib integer-equal to
the oracle's; final_T, colour, alpha within 1e-4 (README parity bound), objects within 3e-4 (smoke()), depth within
1e-4 * z_far (tests/test_gpu_aux.py); alpha bit-equal to 1 - final_T; every gradient normwise within 1e-3 and no significant
element off (util.grad_error with the float32 oracle as yardstick); a Gaussian no pixel blends has a gradient of exactly
0.0 in every attribute; the first entry of a list has a non-zero one.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import list_edge_scenes as S
from util import grad_error

pytestmark = pytest.mark.gpu

RGB_TOL, OBJ_TOL, GRAD_TOL = 1e-4, 3e-4, 1e-3
RAW_GEO = ("_xyz", "_opacity", "_scaling", "_rotation")


def _D():
    import diff_gaussian_rasterization as D
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    D._load()
    return D


def _forms(D):
    """name -> (flags, surface, objects, aux, loss terms).  Every flag value once; the segment-related ones (NO_SEGMENTS,
    bwd_split, aux with grad_alpha alone / with grad_depth, colour-only) are run on every single-view scene like the rest."""
    return {
        "default-raw": (0, "raw", False, False, "C"),
        "default-classic-obj": (0, "classic", True, False, "CO"),
        "fwd1-classic-obj": (D.flag_fwd_split(1), "classic", True, False, "CO"),
        "fwd2-raw-alpha": (D.flag_fwd_split(2), "raw", False, True, "CA"),
        "fwd4-raw": (D.flag_fwd_split(4), "raw", False, False, "C"),
        "fwd1-shared-classic": (D.flag_fwd_split(1) | D.FLAG_FWD_SHARED, "classic", False, False, "C"),
        "fwd2-shared-raw-obj": (D.flag_fwd_split(2) | D.FLAG_FWD_SHARED, "raw", True, False, "CO"),
        "bwd2-raw": (D.flag_bwd_split(2), "raw", False, False, "C"),
        "bwd4-raw-alpha": (D.flag_bwd_split(4), "raw", False, True, "CA"),
        "bwd2-classic-depth": (D.flag_bwd_split(2), "classic", False, True, "CDA"),
        "map0-classic": (D.flag_tile_map(0), "classic", False, False, "C"),
        "map1-raw": (D.flag_tile_map(1), "raw", False, False, "C"),
        "map2-raw-obj": (D.flag_tile_map(2), "raw", True, False, "CO"),
        "map3-classic-alpha": (D.flag_tile_map(3), "classic", False, True, "CA"),
        "noseg-raw": (D.FLAG_NO_SEGMENTS, "raw", False, False, "C"),
        "noseg-classic-obj": (D.FLAG_NO_SEGMENTS, "classic", True, False, "CO"),
        "depth-raw": (0, "raw", False, True, "CDA"),
        "alpha-raw-objmap": (0, "raw", True, True, "CA"),
        "colour-only-raw": (0, "colour", False, False, "C"),
        "colour-only-bwd4": (D.flag_bwd_split(4), "colour", False, False, "C"),
        "colour-only-noseg": (D.FLAG_NO_SEGMENTS, "colour", False, False, "C"),
    }


FORM_NAMES = ["default-raw", "default-classic-obj", "fwd1-classic-obj", "fwd2-raw-alpha", "fwd4-raw", "fwd1-shared-classic",
              "fwd2-shared-raw-obj", "bwd2-raw", "bwd4-raw-alpha", "bwd2-classic-depth", "map0-classic", "map1-raw",
              "map2-raw-obj", "map3-classic-alpha", "noseg-raw", "noseg-classic-obj", "depth-raw", "alpha-raw-objmap",
              "colour-only-raw", "colour-only-bwd4", "colour-only-noseg"]


def seg_shift():
    v = int(os.environ.get("GSR_SEG_SHIFT", "8"))
    return v if 6 <= v <= 16 else 8


def run_single(D, sc, flags, surface, obj, aux, terms, dev, tile_windows=None):
    """One forward + backward on view 0 (tile_windows: loss weights zero outside them).  -> (outputs dict on the CPU,
    gradients dict name -> tensor)."""
    cam = sc.cams[0]
    st = S.settings(cam, torch.tensor(S.BG), D.GaussianRasterizationSettings, device=dev)
    raw = {k: v.to(dev) for k, v in sc.raw.items()}
    w = {k: v.to(dev) for k, v in S.loss_weights(sc, 0, tile_windows).items()}
    with D.extra_flags(flags):
        if surface == "classic":
            act = {k: v.detach().clone().requires_grad_(True) for k, v in S.activate(raw).items()}
            m2d = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
            out = D.GaussianRasterizer(raster_settings=st)(means3D=act["means3D"], means2D=m2d, opacities=act["opacities"],
                                                           shs=act["shs"], sh_objs=act["sh_objs"] if obj else None,
                                                           scales=act["scales"], rotations=act["rotations"], aux=aux)
            leaf = dict(act, means2D=m2d)
            if not obj:
                leaf.pop("sh_objs")
        else:
            colour = surface == "colour"
            leaf = {k: v.detach().clone().requires_grad_(not colour or k in ("_features_dc", "_features_rest"))
                    for k, v in raw.items()}
            m2d = torch.zeros(sc.P, 3, device=dev, requires_grad=not colour)
            out = D.rasterize_gaussians_raw(leaf["_xyz"], m2d, leaf["_features_dc"], leaf["_features_rest"],
                                            leaf["_objects_dc"] if obj else None, leaf["_opacity"], leaf["_scaling"],
                                            leaf["_rotation"], st, aux=aux)
            if colour:
                leaf = {k: leaf[k] for k in ("_features_dc", "_features_rest")}
            else:
                leaf["means2D"] = m2d
                if not obj:
                    leaf.pop("_objects_dc")
        loss = (out[0] * w["C"]).sum()
        if "O" in terms:
            loss = loss + (out[2] * w["O"]).sum()
        if "D" in terms:
            loss = loss + (out[3][0] * w["D"]).sum()
        if "A" in terms:
            loss = loss + (out[4][0] * w["A"]).sum()
        loss.backward()
        torch.cuda.synchronize()
    T = ((sc.W + 15) // 16) * ((sc.H + 15) // 16)
    rg = D.export_state(out[0], "ranges").view(-1, 2).long().cpu()
    res = dict(color=out[0].detach().cpu(), objects=out[2].detach().cpu() if obj else None,
               depth=out[3][0].detach().cpu() if aux else None, alpha=out[4][0].detach().cpu() if aux else None,
               n_contrib=D.export_state(out[0], "n_contrib").view(sc.H, sc.W).long().cpu(),
               final_T=D.export_state(out[0], "final_T").view(sc.H, sc.W).cpu(),
               lens=(rg[:, 1] - rg[:, 0])[:T].numpy(), records=int(D.export_state(out[0], "dv").cpu().long()[5] & 0xFFFFFFFF))
    grads = {k: (v.grad.detach().cpu() if v.grad is not None else None) for k, v in leaf.items()}
    return res, grads


def check_forward(tag, sc, view, res, r64, r32, flags_noseg, worst):
    f = sc.facts[view]
    # (the default footprint cull: the designed lengths are those of the pairs it keeps -- in these scenes all of them,
    # tests/test_list_edges_cpu.py -- so n_contrib below is a position in the oracle's list as well)
    assert np.array_equal(res["lens"].reshape(f.tile_len.shape), f.tile_len_cull), f"{tag}: list lengths differ from the designed ones"
    if not flags_noseg and res.get("records") is not None:
        want = S.records(f.tile_len_cull, seg_shift())
        assert res["records"] == want, f"{tag}: {res['records']} boundary records, designed lengths give {want}"
    bad = res["n_contrib"] != r64.n_contrib
    if bool(bad.any()):
        y, x = [int(t[0]) for t in torch.nonzero(bad, as_tuple=True)]
        raise AssertionError(f"{tag}: n_contrib differs at {int(bad.sum())} pixels, first ({x}, {y}): device "
                             f"{int(res['n_contrib'][y, x])}, oracle {int(r64.n_contrib[y, x])}")
    e = lambda a, b: (a.double() - b.double()).abs().max().item()
    figs = dict(final_T=(e(res["final_T"], r64.final_T), e(r32.final_T, r64.final_T), RGB_TOL),
                colour=(e(res["color"], r64.color), e(r32.color, r64.color), RGB_TOL))
    if res["objects"] is not None:
        figs["objects"] = (e(res["objects"], r64.objects), e(r32.objects, r64.objects), OBJ_TOL)
    if res["alpha"] is not None:
        assert torch.equal(res["alpha"], 1.0 - res["final_T"]), f"{tag}: alpha is not 1 - final_T bit for bit"
        figs["alpha"] = (e(res["alpha"], r64.alpha), e(r32.alpha, r64.alpha), RGB_TOL)
        figs["depth/z_far"] = (e(res["depth"], r64.depth) / r64.z_far, e(r32.depth, r64.depth) / r64.z_far, RGB_TOL)
    print(f"[{tag}] " + ", ".join(f"{k} {v[0]:.2e} (f32 oracle {v[1]:.2e})" for k, v in figs.items()))
    for k, v in figs.items():
        worst[k] = max(worst.get(k, 0.0), v[0])
        assert v[0] <= v[2], f"{tag}: {k} error {v[0]:.3e} > {v[2]:.0e}"


def check_grads(tag, grads, ref64, ref32, dead, first, worst):
    """grads / ref64 / ref32: name -> tensor.  dead: [P] bool; first: indices of first list entries."""
    line = []
    for k, g in grads.items():
        if g is None:                                  # (autograd hands back nothing where the library wrote nothing)
            assert float(ref64[k].abs().max()) == 0.0, f"{tag}: no gradient for {k}"
            continue
        norm, frac = grad_error(g, ref64[k], yard=ref32[k])
        n32, _ = grad_error(ref32[k], ref64[k])
        line.append(f"{k} {norm:.1e}/{frac:.1e} (f32 oracle {n32:.1e})")
        worst[k] = max(worst.get(k, 0.0), norm)
        assert norm <= GRAD_TOL, f"{tag}: grad {k} normwise rel err {norm:.3e}"
        assert frac == 0.0, f"{tag}: grad {k}: {frac:.2e} of the significant elements off"
        if dead is not None and dead.any() and g.shape[0] == dead.shape[0]:
            z = g[torch.from_numpy(dead)].abs().max().item()
            assert z == 0.0, f"{tag}: grad {k}: a Gaussian that no pixel blends received {z:.3e}"
    print(f"[{tag}] grads norm/frac: " + ", ".join(line))
    for k in ("_opacity", "opacities", "_features_dc", "shs"):
        if k in grads and len(first):
            g = grads[k].reshape(grads[k].shape[0], -1)[first]
            assert bool((g != 0).any(dim=1).all()), f"{tag}: a list's first entry has a zero {k} gradient"


def refs_for(sc, view, terms, names, tile_windows=None):
    r64, r32 = S.oracle_run(sc, view, tile_windows=tile_windows), S.oracle_run(sc, view, torch.float32, tile_windows=tile_windows)
    return ({k: S.grad_sum(r64, terms, k) for k in names}, {k: S.grad_sum(r32, terms, k) for k in names})


def first_entries(f):
    return sorted({int(ids[0]) for ids in f.lists.values()})


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    print("\n[list edges] worst errors against the float64 oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(w.items())))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("key", list(S.SINGLE_VIEW))
def test_single_view_forms_against_the_float64_oracle(key, form, worst):
    D = _D()
    dev = torch.device("cuda:0")
    sc = S.get(key)
    flags, surface, obj, aux, terms = _forms(D)[form]
    res, grads = run_single(D, sc, flags, surface, obj, aux, terms, dev)
    r64, r32 = S.oracle_run(sc, 0), S.oracle_run(sc, 0, torch.float32)
    tag = f"{sc.name} / {form}"
    check_forward(tag, sc, 0, res, r64, r32, bool(flags & D.FLAG_NO_SEGMENTS), worst)
    ref64, ref32 = refs_for(sc, 0, terms, list(grads))
    check_grads(tag, grads, ref64, ref32, S.dead_gaussians(sc), first_entries(sc.facts[0]), worst)


@pytest.mark.parametrize("key", list(S.SINGLE_VIEW))
def test_list_lengths_without_the_footprint_cull(key):
    D = _D()
    dev = torch.device("cuda:0")
    sc = S.get(key)
    res, _ = run_single(D, sc, D.FLAG_NO_CULL, "raw", False, False, "C", dev)
    f = sc.facts[0]
    assert np.array_equal(res["lens"].reshape(f.tile_len.shape), f.tile_len)
    assert res["records"] == S.records(f.tile_len, seg_shift())
    assert torch.equal(res["n_contrib"], S.oracle_run(sc, 0).n_contrib)


BATCH_FORMS = ["default", "bwd2", "bwd4", "noseg", "fwd1", "fwd2", "fwd1-shared", "fwd2-shared", "fwd4-map0", "map1", "map2", "map3",
               "aux-alpha", "aux-depth", "colour-only", "objects"]


def _batch_flags(D, name):
    return {"default": 0, "bwd2": D.flag_bwd_split(2), "bwd4": D.flag_bwd_split(4), "noseg": D.FLAG_NO_SEGMENTS,
            "fwd1": D.flag_fwd_split(1), "fwd2": D.flag_fwd_split(2),
            "fwd1-shared": D.flag_fwd_split(1) | D.FLAG_FWD_SHARED, "fwd2-shared": D.flag_fwd_split(2) | D.FLAG_FWD_SHARED,
            "fwd4-map0": D.flag_fwd_split(4) | D.flag_tile_map(0), "map1": D.flag_tile_map(1), "map2": D.flag_tile_map(2), "map3": D.flag_tile_map(3),
            "aux-alpha": 0, "aux-depth": 0, "colour-only": 0, "objects": 0}[name]


# (the per-view backward takes no aux gradients, and a colour-only call has no per-view form of its own to add)
# (`_views` with the segment-related forms and the object channels; the forward-only flags meet the family through `_into`)
BATCH_CASES = [(f, "into") for f in BATCH_FORMS] + [(f, "views") for f in ("default", "bwd2", "bwd4", "noseg", "objects")]


@pytest.mark.parametrize("form,mode", BATCH_CASES, ids=[f"{f}-{m}" for f, m in BATCH_CASES])
@pytest.mark.parametrize("B", [2, 5, 16])
def test_batch_against_the_oracle_of_every_view(B, form, mode, worst):
    """Family D through the batch entry points: every view's forward state against that view's oracle; the `_into` backward
    against the float64 sum over the views, the `_views` backward view by view."""
    batch_case(S.get(("D", B)), B, form, mode, worst)


def batch_case(sc, B, form, mode, worst, oracle=S.oracle_run, first=first_entries):
    """One batch form on a scene of B views.  oracle(sc, view): the float64 result check_forward compares with;
    first(facts of a view): Gaussians whose opacity and colour gradients must not be zero.  -> (out, leaf, vsp, bset)."""
    D = _D()
    dev = torch.device("cuda:0")
    aux, obj, colour = form.startswith("aux"), form == "objects", form == "colour-only"
    terms = {"aux-alpha": "CA", "aux-depth": "CDA", "objects": "CO"}.get(form, "C")
    flags = _batch_flags(D, form)
    sts = [S.settings(c, torch.tensor(S.BG), D.GaussianRasterizationSettings, device=dev) for c in sc.cams]
    names = ("_features_dc", "_features_rest") if colour else tuple(k for k in S.RAW if obj or k != "_objects_dc")
    leaf = {k: v.to(dev).clone().requires_grad_(k in names) for k, v in sc.raw.items()}
    vsp = None if colour else torch.zeros(B, sc.P, 3, device=dev, requires_grad=True)
    bset = D.GradBucketSet(B, sc.P, dev) if mode == "views" else None
    w = [S.loss_weights(sc, v) for v in range(B)]
    stack_w = lambda c: torch.stack([x[c] for x in w]).to(dev)
    with D.extra_flags(flags):
        out = D.rasterize_gaussians_raw_batch(leaf["_xyz"], vsp, leaf["_features_dc"], leaf["_features_rest"], leaf["_opacity"],
                                              leaf["_scaling"], leaf["_rotation"], sts, grad_bucket=bset,
                                              objects_dc=leaf["_objects_dc"] if obj else None, aux=aux)
        loss = (out[0] * stack_w("C")).sum()
        if obj:
            loss = loss + (out[2] * stack_w("O")).sum()
        if "D" in terms:
            loss = loss + (out[2][:, 0] * stack_w("D")).sum()
        if "A" in terms:
            loss = loss + (out[3][:, 0] * stack_w("A")).sum()
        loss.backward()
        torch.cuda.synchronize()
    H, W = sc.H, sc.W
    T = ((W + 15) // 16) * ((H + 15) // 16)
    rg = D.export_state(out[0], "ranges").view(-1, 2).long().cpu()
    lens = (rg[:, 1] - rg[:, 0]).numpy()
    nc = D.export_state(out[0], "n_contrib").view(B, H, W).long().cpu()
    fT = D.export_state(out[0], "final_T").view(B, H, W).cpu()
    recs = int(D.export_state(out[0], "dv").cpu().long()[5] & 0xFFFFFFFF)
    if not flags & D.FLAG_NO_SEGMENTS:
        assert recs == sum(S.records(f.tile_len_cull, seg_shift()) for f in sc.facts), "boundary records of the batch"
    for v in range(B):
        res = dict(color=out[0][v].detach().cpu(), objects=out[2][v].detach().cpu() if obj else None,
                   depth=out[2][v, 0].detach().cpu() if aux else None, alpha=out[3][v, 0].detach().cpu() if aux else None,
                   n_contrib=nc[v], final_T=fT[v], lens=lens[v * T:(v + 1) * T], records=None)
        check_forward(f"{sc.name} / {form} / {mode} / view {v}", sc, v, res, oracle(sc, v),
                      S.oracle_run(sc, v, torch.float32), True, worst)
    dead = S.dead_gaussians(sc)
    per_view = [refs_for(sc, v, terms, names + (() if colour else ("means2D",))) for v in range(B)]
    if vsp is not None:
        for v in range(B):
            check_grads(f"{sc.name} / {form} / {mode} / view {v}", {"means2D": vsp.grad[v].cpu()}, per_view[v][0], per_view[v][1],
                        ~sc.facts[v].blended, [], worst)
    if mode == "views":
        for v in range(B):
            g = dict(zip(("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"),
                         [t.detach().cpu() for t in bset.bucket(v).slices()]))
            g = {k: t.reshape(sc.raw[k].shape) for k, t in g.items()}
            check_grads(f"{sc.name} / {form} / views / view {v}", g, per_view[v][0], per_view[v][1], ~sc.facts[v].blended,
                        first(sc.facts[v]), worst)
        if obj:
            check_grads(f"{sc.name} / {form} / views / objects", {"_objects_dc": leaf["_objects_dc"].grad.cpu()},
                        {"_objects_dc": sum(p[0]["_objects_dc"] for p in per_view)},
                        {"_objects_dc": sum(p[1]["_objects_dc"] for p in per_view)}, dead, [], worst)
    else:
        g = {k: leaf[k].grad.detach().cpu() for k in names}
        ref64 = {k: sum(p[0][k] for p in per_view) for k in names}
        ref32 = {k: sum(p[1][k] for p in per_view) for k in names}
        check_grads(f"{sc.name} / {form} / into", g, ref64, ref32, dead, first(sc.facts[0]), worst)
    return out, leaf, vsp, bset


@pytest.mark.parametrize("shift", [6, 10])
def test_other_segment_lengths_in_a_fresh_process(shift, tmp_path):
    """GSR_SEG_SHIFT is read once per process: a child process per value (one at a time, each under its own time limit, no
    retry) runs families A and B with the default flags and bwd_split(4); the same assertions run in the child, which
    writes its maxima; a child that fails fails the test."""
    out = tmp_path / f"shift{shift}.json"
    env = dict(os.environ, GSR_SEG_SHIFT=str(shift))
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "list_edge_child.py")
    p = subprocess.run([sys.executable, child, str(out)], env=env, timeout=600, capture_output=True, text=True)
    print(p.stdout[-4000:])
    assert p.returncode == 0, f"GSR_SEG_SHIFT={shift}: child failed\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    got = json.loads(out.read_text())
    assert got["seg_shift"] == shift and got["cases"] == 4
    assert got["records"]["A lengths"] == S.records(S.get("A").facts[0].tile_len, shift)
    assert got["records"]["B stops"] == S.records(S.get("B").facts[0].tile_len, shift)
    for k in ("colour", "final_T"):
        assert got["worst"][k] <= RGB_TOL, (k, got["worst"][k])
    for k in S.RAW:
        if k in got["worst"]:
            assert got["worst"][k] <= GRAD_TOL, (k, got["worst"][k])

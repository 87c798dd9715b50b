"""Adaptive density control's scalar source (csrc/gsr_densify.h) on the CPU: tests/host_math/densify_host.cpp runs it in plain loops
over the header the kernels compile.  Held to the float64 five-pass oracle of tests/densify_cases.py on every case (integers equal,
copies bit-equal, child scales and positions within the derived bounds); the tensor-op branch of GaussianModel.densify_and_prune
is held to the same oracle; the statistics to torch.norm in float64; reset_opacity and refit's schedule to the reference's
constants; the keyed normals to the moments of a standard normal; a stand-alone build runs every case under the address and
undefined-behaviour sanitizers.  No GPU."""
import ctypes
import math
import subprocess

import numpy as np
import pytest
import torch

import densify_cases as DC


@pytest.fixture(scope="module")
def lib():
    return DC.host_lib()


# ---- the host build against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.ALL)
def test_host_build_matches_oracle(lib, name):
    c = DC.case(name)
    got, ref = DC.host_run(name), DC.oracle(name)
    worst = DC.check_against_oracle("host", c, got, ref)
    for k in DC.live_names(c):                                  # every destination element was written
        for a in (got["tensors"][k],) + tuple(got["moments"].get(k, ())):
            assert not (DC.bits(a) == DC.bits(np.float32(DC.SENT))).any(), (name, k)
    assert (got["origin"] >= 0).all() and (got["kind"] >= 0).all() and (got["mask"] <= 1).all()
    # the plan: the codes are the reference-domain classes, the offsets their exclusive sums
    code, offs, counts = DC.host_plan(c)
    assert np.array_equal(code, c.expected_codes()), name
    for bit, off, n in zip((DC.KEEP, DC.CLONE, DC.KIDS), offs, counts):
        f = (code & bit) != 0
        assert np.array_equal(off[:-1], np.cumsum(f) - f) and off[-1] == n == int(f.sum())
    print(f"densify host {name}: rows {c.P} -> {got['rows']} {counts}, position error / bound {worst:.3f}")


def test_order_is_the_references(lib):
    """kept originals in row order, clones in parent order, children j-major"""
    c, got = DC.case("mask-N3"), DC.host_run("mask-N3")
    nk, nc, ns = got["counts"]
    o, k = got["origin"], got["kind"]
    assert (k[:nk] == 0).all() and (np.diff(o[:nk]) > 0).all()
    assert (k[nk:nk + nc] == 1).all() and (np.diff(o[nk:nk + nc]) > 0).all()
    for j in range(3):
        seg = slice(nk + nc + j * ns, nk + nc + (j + 1) * ns)
        assert (k[seg] == 2 + j).all() and np.array_equal(o[seg], o[nk + nc:nk + nc + ns]) and (np.diff(o[seg]) > 0).all()
    assert ns >= 30 and nc >= 30


def test_fused_prune_has_no_new_rows(lib):
    """n_clone = n_split = 0: every output row is a kept row with its moments"""
    got = DC.host_run("mix-none-hot")
    assert got["counts"][1:] == [0, 0] and (got["kind"] == 0).all() and 0 < got["rows"] < 777
    c = DC.case("mix-none-hot")
    for k, (m, v) in got["moments"].items():
        assert DC.same(m, c.moments[k][0][got["origin"]]) and DC.same(v, c.moments[k][1][got["origin"]])
    assert DC.host_run("mix-all-pruned")["rows"] == 0


def test_nonfinite_rows(lib):
    c, got = DC.case("nonfinite"), DC.host_run("nonfinite")
    R = DC.NONFINITE_ROWS
    kinds = lambda r: sorted(got["kind"][got["origin"] == r].tolist())   # noqa: E731
    for r in ("nan_scale_cold", "nan_scale_hot", "nan_opacity", "zero_over_zero"):
        assert kinds(R[r]) == [0], r
    for r in ("inf_grad", "nan_rotation", "zero_quaternion", "inf_xyz"):
        assert kinds(R[r]) == [2, 3], r
    assert kinds(R["neg_inf_scale_hot"]) == [0, 1]
    for r in ("inf_scale_hot", "inf_scale_cold", "overflow_scale"):
        assert kinds(R[r]) == [], r
    xyz = got["tensors"]["xyz"]
    child = lambda r: xyz[(got["origin"] == R[r]) & (got["kind"] >= 2)]   # noqa: E731
    assert np.isnan(child("nan_rotation")).all() and np.isnan(child("zero_quaternion")).all()
    assert np.isposinf(child("inf_xyz")[:, 0]).all() and np.isfinite(child("inf_xyz")[:, 1:]).all()
    assert np.isfinite(child("inf_grad")).all()
    # every other row: bit for bit the case without the bad rows' neighbours changing anything
    plain = (got["kind"] == 0) & ~np.isin(got["origin"], list(R.values()))
    assert plain.sum() >= 40 and DC.same(xyz[plain], c.tensors["xyz"][got["origin"][plain]])


def test_children_of_rows_with_an_infinite_or_overflowing_scale(lib):
    """max_screen_size None: a hot row with +inf in a scale and one with raw scale 100 (expf overflows float32, float64's exp does
    not) split and their children stay.  The child scale is +inf, or the finite raw - c; the positions are infinities (the
    oracle's sign where its finite float64 value lies beyond FLT_MAX: DC.check_against_oracle)"""
    name, R = "nonfinite-open", DC.NONFINITE_ROWS
    c, got, ref = DC.case(name), DC.host_run(name), DC.oracle(name)
    DC.check_against_oracle("host", c, got, ref)
    kinds = lambda r: sorted(got["kind"][got["origin"] == r].tolist())   # noqa: E731
    assert kinds(R["inf_scale_hot"]) == [2, 3] and kinds(R["overflow_scale"]) == [2, 3] and kinds(R["inf_scale_cold"]) == [0]
    m = (got["origin"] == R["inf_scale_hot"]) & (got["kind"] >= 2)
    assert np.isposinf(got["tensors"]["scaling"][m][:, 1]).all() and np.isfinite(got["tensors"]["scaling"][m][:, [0, 2]]).all()
    assert np.isinf(got["tensors"]["xyz"][m]).all() and np.array_equal(got["tensors"]["xyz"][m], ref["tensors"]["xyz"][m])
    m = (got["origin"] == R["overflow_scale"]) & (got["kind"] >= 2)
    assert (got["tensors"]["scaling"][m][:, 0] == np.float32(100.0) - np.float32(math.log(1.6))).all()
    assert np.isfinite(ref["tensors"]["xyz"][m]).all() and (np.abs(ref["tensors"]["xyz"][m]) > DC.FLT_MAX).all()
    assert np.array_equal(got["tensors"]["xyz"][m], np.sign(ref["tensors"]["xyz"][m]) * np.inf)


def test_thresholds_are_formed_in_double_and_rounded_once(lib):
    from gsplat_attack import densify as DZ
    out = np.zeros(6, np.float32)
    for mg, mo, ex, pd, N in ((0.0002, 0.005, 4.0, 0.01, 2), (0.0002, 0.005, 5.3, 0.01, 3), (1e-3, 0.3, 0.7, 0.02, 8), (0.0, 0.5, 1.0, 1.0, 1)):
        assert lib.dh_thresholds(mg, mo, ex, pd, 20.0, N, 1, out.ctypes.data) == 0
        want = [mg, math.log(pd * ex), math.log(0.1 * ex), math.log(mo / (1 - mo)), math.log(0.8 * N)]
        assert out[:5].tolist() == [float(np.float32(w)) for w in want]
        py = DZ.thresholds(mg, mo, ex, pd, N)
        assert [py[k] for k in ("max_grad", "t_dense", "t_world", "t_opac", "c")] == out[:5].tolist()
    for kw, rc, word in ((dict(mg=float("nan")), 1, "max_grad"), (dict(ex=0.0), 2, "extent"), (dict(pd=0.0), 2, "extent"), (dict(ex=float("inf")), 2, "extent"),
                         (dict(mo=0.0), 3, "min_opacity"), (dict(mo=1.0), 3, "min_opacity"), (dict(N=0), 4, "N="), (dict(N=9), 4, "N=")):
        a = dict(mg=0.0002, mo=0.005, ex=4.0, pd=0.01, N=2)
        a.update(kw)
        assert lib.dh_thresholds(a["mg"], a["mo"], a["ex"], a["pd"], 20.0, a["N"], 0, None) == rc, kw
        with pytest.raises(ValueError, match=word):
            DZ.thresholds(a["mg"], a["mo"], a["ex"], a["pd"], a["N"])
    assert lib.dh_thresholds(0.0002, 0.005, 4.0, 0.01, float("inf"), 2, 1, None) == 5
    with pytest.raises(ValueError, match="max_screen_size"):
        DZ.thresholds(0.0002, 0.005, 4.0, 0.01, 2, float("inf"))
    with pytest.raises(ValueError, match="screen_prune"):                 # as the binding refuses it
        DZ.thresholds(0.0002, 0.005, 4.0, 0.01, 2, None, True)


def test_build_rotation_is_the_references(lib):
    """utils/general_utils.py:78-99 in float64, entries within e_R = 24 u (tests/densify_cases.py)"""
    r = np.random.default_rng(3)
    for _ in range(200):
        q = (r.normal(0, 1, 4) * math.exp(r.normal(0, 2))).astype(np.float32)
        R = np.zeros(9, np.float32)
        lib.dh_rotation(q.ctypes.data, R.ctypes.data)
        want = DC.build_rotation64(torch.from_numpy(q.astype(np.float64))[None])[0].numpy().reshape(-1)
        assert np.abs(R - want).max() <= 24 * DC.U


# ---- the refusals of the host build --------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_build(lib):
    c = DC.case("mask")
    code, offs, counts = DC.host_plan(c)
    x = c.tensors["xyz"]
    Pn = counts[0] + counts[1] + c.N * counts[2]
    out = np.zeros((Pn, 3), np.float32)
    one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)   # noqa: E731

    def call(n=1, N=2, P=c.P, cnt=counts, src=None, dst=None, cols=3, role=0, origin=None, kind=None):
        return lib.dh_apply(code.ctypes.data, *[o.ctypes.data for o in offs], P, (ctypes.c_int64 * 3)(*cnt), n, src or one(x), dst or one(out),
                            None, None, None, None, (ctypes.c_int32 * 1)(cols), (ctypes.c_int32 * 1)(role), c.tensors["rotation"].ctypes.data, N,
                            0, None, None, None, origin, kind)
    assert call() == 0
    for kw in (dict(N=0), dict(N=9), dict(n=9), dict(n=-1), dict(cols=0), dict(cols=49), dict(role=3), dict(role=1, cols=4), dict(P=(1 << 28) + 1),
               dict(cnt=[c.P + 1, 0, 0]), dict(cnt=[-1, 0, 0]), dict(dst=one(x)), dict(origin=out.ctypes.data),
               dict(P=1 << 28, cnt=[(1 << 28) - 1, (1 << 28) - 1, 0])):
        assert call(**kw) == 1, kw
    z = np.zeros(c.P, np.float32)
    bad = lambda **kw: lib.dh_plan(z.ctypes.data, z.ctypes.data, c.tensors["scaling"].ctypes.data, z.ctypes.data, None, c.P,   # noqa: E731
                                   kw.get("mg", 1.0), kw.get("mo", 0.5), kw.get("ex", 1.0), 0.01, 0.0, kw.get("N", 2), kw.get("flags", 0),
                                   code.ctypes.data, *[o.ctypes.data for o in offs], (ctypes.c_int64 * 3)())
    for kw in (dict(mg=float("inf")), dict(mo=0.0), dict(ex=0.0), dict(N=0), dict(flags=4), dict(flags=2)):
        assert bad(**kw) == 1, kw


# ---- the statistics --------------------------------------------------------------------------------------------------------------------
def test_statistics_against_torch_norm_in_float64(lib):
    r = np.random.default_rng(11)
    P, B = 1000, 4
    grad = (r.normal(0, 1e-3, (B, P, 3)) * np.exp(r.normal(0, 2, (B, P, 1)))).astype(np.float32)
    radii = (r.integers(0, 60, (B, P)) * (r.random((B, P)) < 0.7)).astype(np.int32)
    accum, denom, maxr = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    assert lib.dh_stats(grad.ctypes.data, radii.ctypes.data, None, B, P, accum.ctypes.data, denom.ctypes.data, maxr.ctypes.data) == 0
    seen = torch.from_numpy(radii > 0)
    norm = torch.norm(torch.from_numpy(grad).double()[:, :, :2], dim=-1)                       # the reference's line :711
    want = (norm * seen).sum(0).numpy()
    # per view: the two products and their sum (relative 2 u under the root, so u on it), the root (u), the addition (u)
    assert (np.abs(accum - want) <= 4 * B * DC.U * want + 1e-45).all()
    assert np.array_equal(denom, seen.sum(0).numpy().astype(np.float32)) and np.array_equal(maxr, radii.max(0).astype(np.float32))
    assert (denom == 0).sum() >= 1 and (denom == B).sum() >= 100
    # a batch is B single calls in view order, bit for bit; and the model's tensor-op branch gives the same bits
    a1, d1, m1 = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32)
    for b in range(B):
        assert lib.dh_stats(grad[b].ctypes.data, radii[b].ctypes.data, None, 1, P, a1.ctypes.data, d1.ctypes.data, m1.ctypes.data) == 0
    assert DC.same(a1, accum) and DC.same(d1, denom) and DC.same(m1, maxr)
    from gsplat_attack.gaussian_model import GaussianModel
    m = GaussianModel(0)
    m._xyz = torch.zeros(P, 3)
    m.add_densification_stats(torch.from_numpy(grad), None, radii=torch.from_numpy(radii))
    assert DC.same(m.xyz_gradient_accum.numpy(), accum) and DC.same(m.denom.numpy(), denom) and DC.same(m.max_radii2D.numpy(), maxr)
    flt = r.random((B, P)) < 0.5                                # an explicit filter, no radii: the reference's signature
    a2, d2 = np.zeros(P, np.float32), np.zeros(P, np.float32)
    assert lib.dh_stats(grad.ctypes.data, None, flt.astype(np.uint8).ctypes.data, B, P, a2.ctypes.data, d2.ctypes.data, None) == 0
    m = GaussianModel(0)
    m._xyz = torch.zeros(P, 3)
    for b in range(B):
        leaf = torch.zeros(P, 3, requires_grad=True)
        leaf.grad = torch.from_numpy(grad[b])
        m.add_densification_stats(leaf, torch.from_numpy(flt[b]))
    assert DC.same(m.xyz_gradient_accum.numpy(), a2) and DC.same(m.denom.numpy(), d2) and not m.max_radii2D.any()


# ---- the keyed normals ----------------------------------------------------------------------------------------------------------------
def test_keyed_normals_have_the_moments_of_a_standard_normal(lib):
    """n = 2^18 samples; bounds at six standard errors: mean sqrt(1 / n); variance sqrt(2 / n); fourth moment sqrt(96 / n)
    (Var z^4 = E z^8 - 9 = 96); the share beyond 3 sigma p = 0.0026998: sqrt(p (1 - p) / n).  The smallest uniform is 2^-24, so
    |z| <= 5.77: that cuts 8e-9 of the mass and 1e-5 of the fourth moment, far inside the bounds."""
    P, N = 1 << 14, 8
    z = DC.host_normals(1234, P, N)[:, :, :2].reshape(-1).astype(np.float64)       # 2^18: both members of a Box-Muller pair
    n = z.size
    assert n == 1 << 18
    assert abs(z.mean()) <= 6 * math.sqrt(1 / n)
    assert abs(z.var() - 1) <= 6 * math.sqrt(2 / n)
    assert abs((z ** 4).mean() - 3) <= 6 * math.sqrt(96 / n)
    p = 0.0026997960632601866
    assert abs((np.abs(z) > 3).mean() - p) <= 6 * math.sqrt(p * (1 - p) / n)
    z3 = DC.host_normals(1234, 1 << 16, 4)[:, :, 2].reshape(-1).astype(np.float64)  # the third axis: the second pair's cosine
    assert abs(z3.mean()) <= 6 * math.sqrt(1 / n) and abs(z3.var() - 1) <= 6 * math.sqrt(2 / n)
    full = DC.host_normals(1234, P, N).astype(np.float64)
    for a, b in ((0, 1), (0, 2), (1, 2)):                       # axes of one child: uncorrelated, standard error sqrt(1 / (P N))
        assert abs((full[:, :, a] * full[:, :, b]).mean()) <= 6 * math.sqrt(1 / (P * N))
    assert abs((full[:-1, 0, 0] * full[1:, 0, 0]).mean()) <= 6 * math.sqrt(1 / P)      # neighbouring rows


def test_keyed_normals_depend_on_seed_row_child_axis_only(lib):
    from gsplat_attack import densify as DZ
    a = DC.host_normals(7, 100, 3)
    b = DC.host_normals(7, 6151, 3)
    assert DC.same(a, b[:100])                                  # whatever P is
    assert DC.same(DC.host_normals(7, 10, 3, row0=90), a[90:])
    assert DC.same(DC.host_normals(7, 100, 8)[:, :3], a)        # whatever N is
    assert lib.dh_normal(7, 42, 1, 2) == a[42, 1, 2]
    assert not DC.same(DC.host_normals(8, 100, 3), a)
    u = np.array([lib.dh_uniform(7, r, 0, 0, 0) for r in range(2000)])
    assert (u > 0).all() and (u < 1).all() and abs(u.mean() - 0.5) <= 6 * math.sqrt(1 / 12 / 2000)
    # the Python restatement (the tensor-op branch's): the same uniforms, sine and cosine; only the logarithm may differ (1 ulp each)
    py = DZ.keyed_normals(7, np.arange(6151), 3)
    assert np.abs(py.astype(np.float64) - b).max() <= 4 * DC.U * 5.77


# ---- the tensor-op branch of GaussianModel.densify_and_prune --------------------------------------------------------------------------
SHAPES = dict(xyz=(3,), f_dc=(1, 3), f_rest=(-1, 3), opacity=(1,), scaling=(3,), rotation=(4,), obj_dc=(1, 16))
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation",
            obj_dc="_objects_dc")


def model_of(c, rows=None):
    """a host GaussianModel holding the case: the optimiser of training_setup with the case's moments as its state, the case's row
    mask (or a row range) as its selection, the case's statistics"""
    from gsplat_attack.gaussian_model import GaussianModel
    from gsplat_attack.optim import OptimizationParams
    t = {n: torch.from_numpy(np.array(a)).reshape((c.P,) + tuple(a.shape[1] // 3 if d == -1 else d for d in SHAPES[n])) for n, a in c.tensors.items()}
    m = GaussianModel.from_tensors(t["xyz"], t["f_dc"], t["f_rest"], t["scaling"], t["rotation"], t["opacity"], t["obj_dc"])
    if "obj_dc" not in c.moments and c.moments:
        m._objects_dc.requires_grad = False
    m._setup_optimizer(OptimizationParams(percent_dense=DC.PERCENT_DENSE), row_mask=None if c.mask is None or rows else torch.from_numpy(c.mask.copy()),
                       rows=rows)
    for n, (a, b) in c.moments.items():
        m.optimizer.state[n] = dict(exp_avg=torch.from_numpy(np.array(a)).reshape(t[n].shape), exp_avg_sq=torch.from_numpy(np.array(b)).reshape(t[n].shape))
    m.xyz_gradient_accum = torch.from_numpy(np.array(c.accum))[:, None]
    m.denom = torch.from_numpy(np.array(c.denom))[:, None]
    m.max_radii2D = torch.from_numpy(np.array(c.radii))
    return m


def model_result(c, m, origin, kind):
    Pn = int(origin.numel())
    flat = lambda n, t: t.detach().numpy().reshape(Pn, c.tensors[n].shape[1])   # noqa: E731
    tensors = {n: flat(n, getattr(m, ATTR[n])) for n in DC.NAMES}
    moments = {n: (flat(n, st["exp_avg"]), flat(n, st["exp_avg_sq"])) for n, st in m.optimizer.state.items()}
    mask = m.optimizer.row_mask.numpy() if m.optimizer.row_mask is not None else np.ones(Pn, np.uint8)
    return dict(tensors=tensors, moments=moments, origin=origin.numpy(), kind=kind.numpy(), mask=mask, rows=Pn)


@pytest.mark.parametrize("name", DC.ALL)
def test_cpu_branch_matches_oracle(name):
    c = DC.case(name)
    m = model_of(c)
    old = list(m.parameters())
    origin, kind = m.densify_and_prune(DC.MAX_GRAD, DC.MIN_OPACITY, DC.EXTENT, c.max_screen, N=c.N, normals=torch.from_numpy(np.array(c.normals)),
                                       screen_prune=c.screen_prune)
    got = model_result(c, m, origin, kind)
    DC.check_against_oracle("cpu branch", c, got, DC.oracle(name))
    host = DC.host_run(name)
    assert DC.same(got["tensors"]["scaling"], host["tensors"]["scaling"])                     # raw - c: the same single operation
    assert all(p is not q for p in m.parameters() for q in old)                                    # new nn.Parameters: a render cache sees new geometry
    assert m.xyz_gradient_accum.shape == (got["rows"], 1) and not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()
    assert m._objects_dc.requires_grad == ("obj_dc" in c.moments or not c.moments) and m.densify_count == 1
    for g in m.optimizer.param_groups:
        assert g["params"][0] is getattr(m, ATTR[g["name"]])


@pytest.mark.parametrize("rows", [(100, 300), (40, 200)])
def test_cpu_branch_row_range(rows):
    """a row range ending at P and one not ending there: kept rows keep their selection, new rows move (GaussianAdam.append's rule)"""
    c = DC.case("screen-20")
    m = model_of(c, rows=rows)
    origin, kind = m.densify_and_prune(DC.MAX_GRAD, DC.MIN_OPACITY, DC.EXTENT, c.max_screen, N=c.N, normals=torch.from_numpy(np.array(c.normals)))
    live = m.optimizer._live(int(origin.numel()), "cpu").numpy()
    o, k = origin.numpy(), kind.numpy()
    assert np.array_equal(live[k == 0], (o[k == 0] >= rows[0]) & (o[k == 0] < rows[1])) and live[k > 0].all()
    assert (k > 0).sum() >= 50 and (~live).sum() >= 20


def test_cpu_branch_keyed_normals_and_the_seed_counter():
    c = DC.case("N1")
    host = DC.host_run("N1", True)
    a, b = model_of(c), model_of(c)
    a.densify_count = b.densify_count = c.seed
    oa, ka = a.densify_and_prune(DC.MAX_GRAD, DC.MIN_OPACITY, DC.EXTENT, c.max_screen, N=c.N)
    ob, kb = b.densify_and_prune(DC.MAX_GRAD, DC.MIN_OPACITY, DC.EXTENT, c.max_screen, N=c.N, seed=c.seed)
    assert torch.equal(a._xyz, b._xyz) and a.densify_count == c.seed + 1
    ch = host["kind"] >= 2
    e = DC.position_bound(c, host["origin"], host["kind"], DC.host_normals(c.seed, c.P, c.N), keyed=True, factor=2.0)
    assert (np.abs(a._xyz.detach().numpy()[ch].astype(np.float64) - host["tensors"]["xyz"][ch]) <= e).all()
    other = model_of(c)
    other.densify_and_prune(DC.MAX_GRAD, DC.MIN_OPACITY, DC.EXTENT, c.max_screen, N=c.N, seed=c.seed + 1)
    assert not torch.equal(other._xyz, a._xyz)


def test_prune_points_on_the_host():
    c = DC.case("mask")
    m = model_of(c)
    sel = torch.from_numpy(np.random.default_rng(2).random(c.P) < 0.3)
    m.prune_points(sel)
    keep = ~sel
    assert m._xyz.shape[0] == int(keep.sum()) and torch.equal(m._xyz.detach(), torch.from_numpy(np.array(c.tensors["xyz"]))[keep])
    assert DC.same(m.optimizer.state["f_rest"]["exp_avg"].numpy().reshape(int(keep.sum()), -1), c.moments["f_rest"][0][keep.numpy()])
    assert DC.same(m.xyz_gradient_accum.numpy(), c.accum[keep.numpy()]) and DC.same(m.max_radii2D.numpy(), c.radii[keep.numpy()])
    assert np.array_equal(m.optimizer.row_mask.numpy(), c.mask[keep.numpy()])


# ---- reset_opacity, oneupSHdegree and refit's schedule ----------------------------------------------------------------------------------
def test_reset_opacity_is_the_references():
    c = DC.case("state-frozen")
    m = model_of(c)
    before = m._opacity.detach().clone()
    sched = m.optimizer.state["xyz"]["exp_avg"].clone()
    m.reset_opacity()
    x = torch.min(torch.sigmoid(before), torch.ones_like(before) * 0.01)                       # :414
    assert torch.equal(m._opacity.detach(), torch.log(x / (1 - x)))
    assert float(m.get_opacity.detach().max()) <= 0.01 + 1e-9 and (m.get_opacity.detach() < 0.0099).sum() >= 30
    st = m.optimizer.state["opacity"]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and torch.equal(m.optimizer.state["xyz"]["exp_avg"], sched)     # :563-564
    assert m.optimizer.param_groups[3]["params"][0] is m._opacity


def test_oneupSHdegree_stops_at_the_maximum():
    from gsplat_attack.gaussian_model import GaussianModel
    m = GaussianModel(3)
    m.active_sh_degree = 0
    for want in (1, 2, 3, 3):
        m.oneupSHdegree()
        assert m.active_sh_degree == want


def test_schedule_is_the_references():
    """arguments/__init__.py:82-88 and the constants of the original training loop: densify every 100 from 600 to 14900 (after 500,
    before 15000), max_screen_size 20 past iteration 3000, opacity reset every 3000 below 15000, SH degree up every 1000"""
    from gsplat_attack.densify import DensifyParams
    d = DensifyParams()
    assert (d.densify_from_iter, d.densify_until_iter, d.densification_interval, d.opacity_reset_interval, d.densify_grad_threshold) == \
        (500, 15000, 100, 3000, 0.0002)
    assert (d.min_opacity, d.size_threshold, d.sh_degree_interval, d.N) == (0.005, 20.0, 1000, 2)
    acts = {i: d.actions(i) for i in range(1, 16001)}
    dens = [i for i, a in acts.items() if a[1]]
    assert dens == list(range(600, 15000, 100))
    assert [i for i, a in acts.items() if a[2]] == [3000, 6000, 9000, 12000]
    assert [i for i, a in acts.items() if a[0]] == list(range(1000, 16001, 1000))
    assert all(acts[i][3] is None for i in dens if i <= 3000) and all(acts[i][3] == 20.0 for i in dens if i > 3000)
    w = DensifyParams(white_background=True)
    assert [i for i in range(1, 4000) if w.actions(i)[2]] == [500, 3000]


def test_refit_runs_the_schedule_on_a_tiny_host_model(monkeypatch):
    """which iterations densify, reset and raise the degree, and with what arguments: refit's loop with the render and the loss
    replaced by stand-ins (no device here)"""
    from gsplat_attack import image_loss, optim, renderer
    from gsplat_attack.densify import DensifyParams
    c = DC.case("sh1")
    m = model_of(c)
    m.active_sh_degree, m.max_sh_degree = 0, 3
    log = []

    def fake_render(cam, model, pipe, bg):
        P = model._xyz.shape[0]
        vs = torch.zeros(P, 3, requires_grad=True)
        img = (model._xyz.sum() + model._opacity.sum() + vs.sum() * 0.0) * torch.ones(3, 4, 4)
        vs.grad = torch.full((P, 3), 1e-3)
        return dict(render=img, viewspace_points=vs, radii=torch.ones(P, dtype=torch.int32))
    monkeypatch.setattr(renderer, "render", fake_render)
    monkeypatch.setattr(image_loss, "photometric_loss", lambda img, gt, lam: (img - gt).abs().mean())
    for name in ("densify_and_prune", "reset_opacity", "oneupSHdegree", "add_densification_stats"):
        real = getattr(m, name)
        setattr(m, name, (lambda real, name: lambda *a, **k: (log.append((it_of(), name, a[:4] if name == "densify_and_prune" else ())), real(*a, **k))[1])(real, name))
    count = [0]                                     # the 1-based iteration: update_learning_rate opens each one
    real_lr = m.update_learning_rate
    m.update_learning_rate = lambda it: (count.__setitem__(0, it), real_lr(it))[1]
    it_of = lambda: count[0]   # noqa: E731
    dp = DensifyParams(densify_from_iter=3, densify_until_iter=14, densification_interval=4, opacity_reset_interval=6, densify_grad_threshold=0.0002,
                       sh_degree_interval=5, extent=DC.EXTENT)
    losses = optim.refit(m, [None], [torch.zeros(3, 4, 4)], iters=16, densify=dp)
    assert losses.shape == (16,)
    by = lambda n: [i for i, name, _ in log if name == n]   # noqa: E731
    assert by("add_densification_stats") == list(range(1, 14))
    assert by("densify_and_prune") == [4, 8, 12] and by("reset_opacity") == [6, 12] and by("oneupSHdegree") == [5, 10, 15]
    args = {i: a for i, name, a in log if name == "densify_and_prune"}
    assert args[4] == (0.0002, 0.005, DC.EXTENT, None) and args[8] == (0.0002, 0.005, DC.EXTENT, 20.0)
    assert m.active_sh_degree == 3 and m.densify_count == 3 and m._xyz.shape[0] != c.P
    # densify=None: the plain loop, none of the four is called
    log.clear()
    optim.refit(m, [None], [torch.zeros(3, 4, 4)], iters=3)
    assert log == []


# ---- the stand-alone program under the sanitizers -------------------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "densify_host_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DDENSIFY_MAIN", "-I", DC.CSRC, DC.SRC, "-o", exe], check=True)
    data = tmp_path / "calls.bin"
    calls = [(n, keyed) for n in DC.ALL for keyed in ((False, True) if n in ("mask", "size-P65-N3") else (False,))]
    with open(data, "wb") as f:
        f.write(np.array([len(calls)], np.int32).tobytes())
        for name, keyed in calls:
            c = DC.case(name)
            names = DC.live_names(c)
            f.write(np.array([c.P], np.int64).tobytes())
            f.write(np.array([c.N, c.flags(), len(names), not keyed, c.mask is not None, c.seed], np.int32).tobytes())
            f.write(np.array([DC.MAX_GRAD, DC.MIN_OPACITY, DC.EXTENT, DC.PERCENT_DENSE, c.max_screen or 0.0], np.float64).tobytes())
            for a in (c.accum, c.denom, c.radii, c.tensors["scaling"], c.tensors["opacity"], c.tensors["rotation"]):
                f.write(a.tobytes())
            if not keyed:
                f.write(c.normals.tobytes())
            if c.mask is not None:
                f.write(c.mask.tobytes())
            for k in names:
                f.write(np.array([c.tensors[k].shape[1], DC.ROLES.get(k, DC.COPY), k in c.moments], np.int32).tobytes())
                f.write(c.tensors[k].tobytes())
                if k in c.moments:
                    f.write(c.moments[k][0].tobytes() + c.moments[k][1].tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"calls {len(calls)}"
    for i, (name, keyed) in enumerate(calls):       # the same answers as the library the other tests load
        c, h = DC.case(name), DC.host_run(name, keyed)
        head = f"call {i} rows {c.P} counts {h['counts'][0]} {h['counts'][1]} {h['counts'][2]} hash "
        assert lines[i].startswith(head), (name, lines[i])
        if c.P <= 65:                               # the hash of every output, where hashing it here is quick
            flat = []
            for k in DC.live_names(c):
                flat.append(h["tensors"][k])
                if k in h["moments"]:
                    flat += list(h["moments"][k])
            flat += [h["mask"], h["origin"], h["kind"]]
            assert lines[i] == head + str(DC.fnv1a(flat)), name

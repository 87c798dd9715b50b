"""The fused Adam step's scalar source (csrc/gsr_adam.h) on the CPU: tests/host_math/adam_host.cpp runs it in plain loops over the
header the kernel compiles.  Held to torch.optim.Adam (float64, state injected, the derived bounds of tests/adam_cases.py) on
every case; the tensor-op branch of gsplat_attack.optim.GaussianAdam.step() is held to the same oracle; the schedule is
compared with the reference's recorded values; a stand-alone build runs every case under the address and undefined-behaviour
sanitizers.  No GPU."""
import ctypes
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import adam_cases as AC


@pytest.fixture(scope="module")
def lib():
    return AC.host_lib()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


# ---- the host build against torch.optim.Adam -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", AC.SWEEP_COLS)
def test_host_build_matches_oracle_on_the_sweep(lib, cols):
    worst = 0.0
    for rows in AC.SWEEP_ROWS:
        for t in AC.SWEEP_T:
            c = AC.case(AC.sweep_name(cols, rows, t))
            got = AC.host_run(c)
            worst = max(worst, AC.check("host", c, got))
            assert AC.moved_fraction(c, got) >= 0.99, c.name          # a test that compared nothing would fail here
    print(f"adam host sweep cols {cols}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", AC.PACKS + AC.OTHER)
def test_host_build_matches_oracle(lib, name):
    c = AC.case(name)
    print(f"adam host {name}: worst error / bound {AC.check('host', c, AC.host_run(c)):.3f}")


def test_first_step_from_zero_state(lib):
    """t = 1, m = v = 0: m^ = g, sqrt(v^) = |g|, so |dx| = lr |g| / (|g| + eps): within lr (eps / |g| + 16 u) + u |x| of lr
    wherever |g| >= 1e-10 (eps = 1e-15: 1e-5 lr at most; 16 u covers the eight roundings, doubled), and exactly 0 where g = 0"""
    c = AC.case("first-step")
    x, g, _, _ = c.tensors[0]
    (ox, om, ov), = AC.host_run(c)
    zero, big = g == 0.0, np.abs(g) >= 1e-10
    assert zero.sum() >= 150 and big.sum() >= 500
    assert np.array_equal(_bits(ox[zero]), _bits(x[zero])) and not om[zero].any() and not ov[zero].any()
    dx = np.abs(ox.astype(np.float64) - x.astype(np.float64))[big]
    lr = c.lr[0]
    tol = lr * (c.eps[0] / np.abs(g[big]).astype(np.float64) + 16 * AC.U) + AC.U * np.abs(x[big])
    assert (np.abs(dx - lr) <= tol).all(), float(np.max(np.abs(dx - lr) / tol))
    assert np.array_equal(np.sign(ox[big].astype(np.float64) - x[big]), -np.sign(g[big]))


def test_lr_zero_updates_the_moments_only(lib):
    c = AC.case("lr0")
    for (x, g, m, v), (ox, om, ov) in zip(c.tensors, AC.host_run(c)):
        assert np.array_equal(_bits(ox), _bits(x))
        assert (om != m).mean() > 0.99 and (ov != v).mean() > 0.99


@pytest.mark.parametrize("name", AC.NONFINITE)
def test_nonfinite_and_range_agree_with_torch_float32(lib, name):
    """element by element the same class (finite, NaN, +inf, -inf) as torch.optim.Adam on CPU float32 tensors in x, m and v,
    and every other element bit for bit the run without the bad element"""
    c, base = AC.case(name), AC.case("nonfinite-base")
    got, clean = AC.host_run(c)[0], AC.host_run(base)[0]
    ref = AC.oracle(c, torch.float32)[0]
    others = np.ones(c.tensors[0][0].shape, bool)
    others[AC.NONFINITE_AT] = False
    for what, a, r, b in zip("xmv", got, ref, clean):
        assert np.array_equal(AC.classes(a), AC.classes(r)), (name, what, a[AC.NONFINITE_AT], r[AC.NONFINITE_AT])
        assert np.array_equal(_bits(a[others]), _bits(b[others])), (name, what)
    x_in = c.tensors[0][0][AC.NONFINITE_AT]
    if name in ("nonfinite-nan", "nonfinite-+inf", "nonfinite--inf"):
        assert np.isnan(got[0][AC.NONFINITE_AT])
    else:                                       # finite, and the float32 oracle's value to a few ulps of the step
        assert np.isfinite(got[0][AC.NONFINITE_AT])
        assert abs(float(got[0][AC.NONFINITE_AT]) - float(ref[0][AC.NONFINITE_AT])) <= 16 * AC.U * (abs(float(x_in)) + 1.0)
    if "1e-25" in name:                         # the square underflows: v' = b2 v, m' takes the gradient
        assert got[2][AC.NONFINITE_AT] == np.float32(c.b2[0]) * c.tensors[0][3][AC.NONFINITE_AT]
    if "1e19" in name:                          # below sqrt(FLT_MAX) = 1.84e19: g g = 1e38 is finite, v' = 1e35, and x moves
        assert np.isfinite(got[2][AC.NONFINITE_AT]) and got[2][AC.NONFINITE_AT] > 1e34
        assert got[0][AC.NONFINITE_AT] != x_in


def test_gradient_beyond_the_root_of_flt_max(lib):
    """|g| = 5e19 > sqrt(FLT_MAX) = 1.84e19: g g = +inf, v' = +inf, den = +inf, x stays bit for bit and m' takes the gradient
    (csrc/gsr_adam.h).  The stated difference from torch, whose ((1 - b2) g) g is still finite here and moves x"""
    c = AC.beyond_root_case()
    (ox, om, ov), = AC.host_run(c)
    x, g, m, v = c.tensors[0]
    at = AC.NONFINITE_AT
    assert np.isposinf(ov[at]) and ox[at] == x[at] and np.isfinite(om[at]) and om[at] > 1e18
    ref = AC.oracle(c, torch.float32)[0]
    assert np.isfinite(ref[2][at]) and ref[0][at] != x[at]
    others = np.ones(x.shape, bool)
    others[at] = False
    clean = AC.host_run(AC.case("nonfinite-base"))[0]
    for a, b in zip((ox, om, ov), clean):
        assert np.array_equal(_bits(a[others]), _bits(b[others]))


def test_zero_gradient_and_zero_moments_move_nothing(lib):
    z = np.zeros((65, 3), np.float32)
    x = AC._four(AC._rng("zeros"), 65, 3)[0]
    (ox, om, ov), = AC.host_run(AC.Call("zeros", [(x, z, z, z)], 1e-2, 1))
    assert np.array_equal(_bits(ox), _bits(x)) and not om.any() and not ov.any()


# ---- row selection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.SELECT)
def test_mask_and_range(lib, name):
    """rows left out: x, m, v bit for bit their inputs (AC.check); live rows: bit for bit the step without a selection"""
    c = AC.case(name)
    live = c.live(0)
    want = AC.SELECT_LIVE.get(name, len(AC.boundary_rows()))
    assert int(live.sum()) == want and int((~live).sum()) == AC.P_MASK - want, name
    got, full = AC.host_run(c), AC.host_run(c.without_selection())
    AC.check("host", c, got)
    for t in range(c.n):
        for a, b in zip(got[t], full[t]):
            assert np.array_equal(_bits(a[live]), _bits(b[live])), (name, t)
        if live.any():
            assert (got[t][0][live] != c.tensors[t][0][live]).mean() > 0.9


def test_boundary_mask_has_a_live_row_on_either_side_of_every_span_boundary(lib):
    S = AC.span()
    assert S == lib.ah_span() and S % 4 == 0
    rows = set(AC.boundary_rows())
    assert 50 < len(rows) < AC.P_MASK // 4                   # many boundaries, most rows dead
    for cols in AC.MODEL_COLS:
        for b in range(1, int(lib.ah_blocks(AC.P_MASK * cols))):
            assert int(lib.ah_row_of(b * S - 1, cols)) in rows and int(lib.ah_row_of(b * S, cols)) in rows
    # the middle-row case: its workgroup of the one-column tensor (rows 0 .. S-1) holds no other live row
    assert AC.case("mask-middle").live(0).nonzero()[0].tolist() == [AC.P_MASK // 2] and 0 < AC.P_MASK // 2 < S - 1


def test_launch_arithmetic(lib):
    S = AC.span()
    for n in (0, 1, S - 1, S, S + 1, 75 * 10 ** 6, 1 << 33):
        assert lib.ah_blocks(n) == -(-n // S)
    for e, cols in ((0, 1), (44, 45), (45, 45), (46124, 45), (2 ** 33 + 5, 48)):
        assert lib.ah_row_of(e, cols) == e // cols
    r = np.random.default_rng(5)
    for trial in range(300):
        n = int(r.integers(1, AC.MAX_TENSORS + 1))
        blocks = r.integers(0, 4, n) * r.integers(0, 2, n)                       # many tensors without rows, anywhere
        first = np.zeros(AC.MAX_TENSORS + 1, np.uint32)
        first[1:n + 1] = np.cumsum(blocks)
        first[n:] = first[n]
        for b in range(int(first[n])):
            t = lib.ah_tensor_of_block(first.ctypes.data, n, b)
            assert first[t] <= b < first[t + 1] and blocks[t] > 0, (trial, first, b, t)


def test_refusals_of_the_host_build(lib):
    c = AC.case("pack1")
    x, g, m, v = (a.copy() for a in c.tensors[0])
    one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)   # noqa: E731

    def call(n=1, rows=257, cols=3, lr=1e-2, b1=0.9, b2=0.999, eps=1e-15, step=1, mask=None, rb=0, re=-1, px=None):
        return lib.ah_step_multi(n, px or one(x), one(g), one(m), one(v), (ctypes.c_int64 * 1)(rows), (ctypes.c_int32 * 1)(cols),
                                 (ctypes.c_float * 1)(lr), (ctypes.c_float * 1)(b1), (ctypes.c_float * 1)(b2), (ctypes.c_float * 1)(eps),
                                 step, mask, rb, re)
    for kw in (dict(n=0), dict(n=9), dict(step=0), dict(cols=0), dict(cols=49), dict(rows=-1), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0),
               dict(eps=-1e-8), dict(lr=float("nan")), dict(lr=float("inf")), dict(eps=float("inf")), dict(b2=float("nan")),
               dict(rb=-1), dict(rb=5, re=4), dict(re=258), dict(rb=258, re=258), dict(px=(ctypes.c_void_p * 1)(None))):
        assert call(**kw) == 1, kw
    assert np.array_equal(x, c.tensors[0][0]) and np.array_equal(m, c.tensors[0][2])
    assert call(rows=0, px=(ctypes.c_void_p * 1)(None)) == 0 and call(rb=257, re=257) == 0 and call(rb=0, re=0) == 0
    assert np.array_equal(x, c.tensors[0][0])


# ---- trajectories ------------------------------------------------------------------------------------------------------------------
def host_trajectory():
    x0, grads = AC.trajectory_inputs()
    x, m, v = x0.copy(), np.zeros_like(x0), np.zeros_like(x0)
    xs = []
    for k, g in enumerate(grads):
        (x, m, v), = AC.host_run(AC.Call("trajectory", [(x, g, m, v)], AC.TRAJ_LR, k + 1))
        xs.append(x)
    return np.stack(xs)


def test_trajectory_against_torch_float64_and_float32(lib):
    xs = host_trajectory()
    e64, e32 = AC.trajectory_error(xs, torch.float64), AC.trajectory_error(xs, torch.float32)
    print(f"adam host trajectory: worst error / travelled distance vs float64 {e64:.3e}, vs float32 {e32:.3e}")
    assert e64 <= 4 * AC.TRAJ_ERR_VS_F64 and e32 <= 4 * AC.TRAJ_ERR_VS_F32


def test_the_oracle_notices_small_faults(lib):
    """a step with eps dropped from the denominator at the smallest gradients, a moment one step stale, an x moved by 3 bounds"""
    c = AC.case("sweep-c3-r65-t10")
    ref = AC.oracle(c)
    got = AC.host_run(c)
    assert AC.check("host", c, got, ref) <= 1.0
    e_x = AC.bounds(c, 0, ref[0])[0]
    bad = [(got[0][0].astype(np.float64) + 3 * e_x).astype(np.float32), got[0][1], got[0][2]]
    with pytest.raises(AssertionError):
        AC.check("mutant", c, [tuple(bad)], ref)
    stale = AC.host_run(AC.Call("stale", c.tensors, c.lr, c.step + 1))          # the bias corrections of the wrong step
    with pytest.raises(AssertionError):
        AC.check("mutant", c, stale, ref)


# ---- the scalars -----------------------------------------------------------------------------------------------------------------
def test_bias_corrections_are_shared(lib):
    from gsplat_attack import optim
    for lr, b1, b2, t in ((1e-2, 0.9, 0.999, 1), (0.00016, 0.9, 0.999, 2), (0.05, 0.5, 0.9, 10), (1e-3, 0.0, 0.0, 7), (0.0, 0.9, 0.999, 3),
                          (2.5e-3, 0.9, 0.999, 1000), (2.5e-3, 0.9, 0.999, 100000)):
        ss, sb = ctypes.c_float(), ctypes.c_float()
        lib.ah_bias(AC.F32(lr), AC.F32(b1), AC.F32(b2), t, ctypes.byref(ss), ctypes.byref(sb))
        py = optim.bias_corrections(lr, b1, b2, t)
        assert (ss.value, sb.value) == py, (lr, b1, b2, t)
        assert abs(ss.value - AC.F32(lr) / (1 - AC.F32(b1) ** t)) <= AC.U * ss.value
        assert abs(sb.value - math.sqrt(1 - AC.F32(b2) ** t)) <= AC.U * sb.value


def _ulp(v):
    return abs(np.nextafter(v, np.inf) - v)


def test_expon_lr_against_the_reference(lib):
    from gsplat_attack import optim
    gold = np.load(os.path.join(AC.ROOT, "tests", "golden", "ref_adam.npz"))
    steps = gold["steps"].tolist()
    assert steps == [-1, 0, 1, 100, 15000, 30000, 40000]
    for name in ("default", "delayed", "zero"):
        lr_init, lr_final, delay_steps, delay_mult, max_steps = gold[name + "_params"].tolist()
        fn = optim.get_expon_lr_func(lr_init, lr_final, lr_delay_steps=int(delay_steps), lr_delay_mult=delay_mult, max_steps=int(max_steps))
        for s, want in zip(steps, gold[name].tolist()):
            for got in (lib.ah_expon_lr(s, lr_init, lr_final, int(delay_steps), delay_mult, int(max_steps)), fn(s)):
                assert abs(got - want) <= _ulp(want), (name, s, got, want)
    # the fixture is the schedule the set-ups use (exp(log(.)) is not exact: a few ulps)
    assert gold["default"][0] == 0.0 and abs(gold["default"][1] - 0.00016) <= 1e-18 and not gold["zero"].any()
    assert abs(gold["default"][5] - 0.0000016) <= 1e-20 and gold["default"][6] == gold["default"][5]
    assert abs(gold["delayed"][1] - 0.01 * 0.01) <= 1e-18         # delay_mult x lr_init at step 0


# ---- the stand-alone program under the sanitizers -------------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "adam_host_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DADAM_MAIN", "-I", AC.CSRC, AC.SRC, "-o", exe], check=True)
    data = tmp_path / "calls.bin"
    with open(data, "wb") as f:
        f.write(np.array([len(AC.NAMES)], np.int32).tobytes())
        for name in AC.NAMES:
            c = AC.case(name)
            f.write(np.array([c.n, c.mask is not None], np.int32).tobytes())
            f.write(np.array([c.step] + list((0, -1) if c.rows is None else c.rows), np.int64).tobytes())
            for t in range(c.n):
                f.write(np.array([c.tensors[t][0].shape[0]], np.int64).tobytes() + np.array([c.tensors[t][0].shape[1]], np.int32).tobytes())
                f.write(np.array([c.lr[t], c.b1[t], c.b2[t], c.eps[t]], np.float32).tobytes() + np.array([c.shift[t]], np.int32).tobytes())
            if c.mask is not None:
                f.write(c.mask.tobytes())
            for four in c.tensors:
                for a in four:
                    f.write(a.tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"calls {len(AC.NAMES)} lookup 24"
    for k, name in enumerate(AC.NAMES):             # the same answers as the library the other tests load
        c = AC.case(name)
        flat = [a for x, m, v in AC.host_run(c) for a in (x, m, v) if a.size]
        assert lines[k] == f"call {k} tensors {c.n} step {c.step} hash {AC.fnv1a(flat)}", name


# ---- the tensor-op branch of GaussianAdam.step() on the CPU -----------------------------------------------------------------------
def fallback_run(c):
    """every tensor of the call through GaussianAdam.step() on CPU tensors (one optimiser per tensor: the cases have per-tensor
    betas and eps), state injected"""
    from gsplat_attack import optim
    out = []
    for t, (x, g, m, v) in enumerate(c.tensors):
        p = torch.nn.Parameter(torch.from_numpy(x.copy()))
        opt = optim.GaussianAdam(types.SimpleNamespace(_xyz=p), [dict(name="xyz", lr=c.lr[t])], eps=c.eps[t], betas=(c.b1[t], c.b2[t]),
                                 row_mask=None if c.mask is None else torch.from_numpy(c.mask.copy()), rows=c.rows)
        opt.state["xyz"] = dict(exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
        opt.step_count = c.step - 1
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        assert opt.step_count == c.step
        out.append((p.detach().numpy(), opt.state["xyz"]["exp_avg"].numpy(), opt.state["xyz"]["exp_avg_sq"].numpy()))
    return out


@pytest.mark.parametrize("group", ["sweep", "packs", "other", "select"])
def test_cpu_branch_matches_oracle(group):
    """every case within the oracle's bounds.  Against the host build: both moments bit for bit (sums and products, which torch's
    CPU kernels round once like the scalar source); x is not expected to be -- torch's vectorised root and quotient leave one
    or two elements of a case an ulp away -- so its agreement is counted and printed, not asserted"""
    names = dict(sweep=AC.SWEEP, packs=AC.PACKS, other=AC.OTHER, select=AC.SELECT)[group]
    worst = same = 0
    for name in names:
        c = AC.case(name)
        got, host = fallback_run(c), AC.host_run(c)
        worst = max(worst, AC.check("cpu branch", c, got))
        for ga, ha in zip(got, host):
            assert np.array_equal(_bits(ga[1]), _bits(ha[1])) and np.array_equal(_bits(ga[2]), _bits(ha[2])), name
        same += all(np.array_equal(_bits(ga[0]), _bits(ha[0])) for ga, ha in zip(got, host))
    print(f"adam cpu branch {group}: worst error / bound {worst:.3f}; x bit-equal to the host build in {same} of {len(names)} cases")


@pytest.mark.parametrize("name", AC.NONFINITE)
def test_cpu_branch_nonfinite_classes(name):
    c = AC.case(name)
    for a, r in zip(fallback_run(c)[0], AC.oracle(c, torch.float32)[0]):
        assert np.array_equal(AC.classes(a), AC.classes(r)), name

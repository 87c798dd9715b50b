"""The projected-gradient step's scalar source (csrc/gsr_pgd.h) on the CPU: tests/host_math/pgd_host.cpp runs it in plain loops
over the header the kernels compile.  Held to the float64 oracle of tests/pgd_cases.py on every named case and on a fuzz; the
CPU branch of gsplat_attack.pgd (the tensor formulation, which sets the non-finite contract) is held to the same oracle; a
stand-alone build runs every case under the address and undefined-behaviour sanitizers.  No GPU."""
import subprocess

import numpy as np
import pytest
import torch

import pgd_cases as PC


@pytest.fixture(scope="module")
def lib():
    return PC.host_lib()


def _host_check(name, rule):
    c = PC.case(name)
    ref = PC.oracle(c, rule, K=PC.K_NORMED)          # the host build sums the squares in double
    return PC.check("host", c, rule, PC.host_step(c, rule), ref, no_step=PC.no_step(name) if c.either else None, quiet=True)


@pytest.mark.parametrize("cols", range(1, PC.MAX_COLS + 1))
def test_host_build_matches_oracle_on_the_sweep(lib, cols):
    worst = {r: 0.0 for r in PC.RULES}
    for rows in PC.sweep_rows(cols):
        for rule in PC.RULES:
            worst[rule] = max(worst[rule], _host_check(f"sweep-c{cols}-r{rows}", rule))
    print(f"pgd host sweep cols {cols}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name", PC.THRESHOLD + PC.OTHER + PC.MASS + PC.NONFINITE)
def test_host_build_matches_oracle(lib, name):
    c = PC.case(name)
    for rule in c.rules:
        w = _host_check(name, rule)
        print(f"pgd host {name} {rule}: worst error / bound {w:.3f}")


def test_about_half_of_the_sweep_rows_are_clipped():
    n = k = band = 0
    for name in PC.SWEEP:
        ref = PC.oracle(PC.case(name), "l2")
        n, k, band = n + len(ref.clipped), k + int(ref.clipped.sum()), band + int(ref.band.sum())
    print(f"pgd sweep: {n} rows, {k} clipped, {band} within the either-branch band")
    assert 0.35 * n < k < 0.65 * n and band < 0.01 * n


def test_rows_on_the_threshold(lib):
    """d = (3, .., 4) with eps = 5: float32 gives exactly 5, which is not > eps: x comes back bit for bit.  The 4 one ulp up:
    clipped, the formulation moves that component by -4.77e-7.  (PC.check asserts both for every threshold case; here the
    numbers, and that the scaled copies outside the band take the branch the oracle names.)"""
    for name in PC.THRESHOLD:
        c = PC.case(name)
        out = PC.host_step(c, "l2")
        assert np.array_equal(out[0].view(np.uint32), c.x[0].view(np.uint32))
        moved = float(out[1, -1]) - float(c.x[1, -1])
        assert (-3e-7 < moved < -1e-7) if name.startswith("threshold8") else (-6e-7 < moved < -3e-7), (name, moved)
        ref = PC.oracle(c, "l2", K=PC.K_NORMED)
        assert ref.band[:2].all()                                  # both rows are inside the band: the bits above decide
        sure = ~ref.band
        assert sure.sum() >= 20, (name, int(sure.sum()))           # k = 10..20 at least lie outside it
        changed = (out != c.x).any(axis=1)
        assert np.array_equal(changed[sure], ref.clipped[sure]), name


def test_nonfinite_contract_in_numbers(lib):
    """the contract of csrc/gsr_pgd.h, spelled out on the host build (the oracle test above holds every element)"""
    at = PC.NONFINITE_AT
    base = PC.case("nonfinite-base")
    others = np.ones(base.x.shape, bool)
    others[at] = False
    for v in PC.NONFINITE_VALUES:
        res = {(who, rule): PC.host_step(PC.case(f"nonfinite-{who}-{v}"), rule) for who in ("g", "x", "x0") for rule in PC.RULES}
        for key, out in res.items():
            assert np.isfinite(out[others]).all(), (v, key)      # the damage stays in its element
        clean = PC.host_step(base, "linf")
        zero_g = base.g.copy()
        zero_g[at] = 0.0
        # L-inf, gradient: sign(NaN) = 0, sign(+-inf) = +-1: always finite
        want = PC.host_step(base, "linf", g=zero_g if v == "nan" else np.where(others, base.g, 1.0 if v == "+inf" else -1.0))
        assert np.array_equal(res[("g", "linf")], want)
        assert np.array_equal(res[("g", "linf")][others], clean[others])
        # L2, gradient: no step anywhere (the projection alone); a NaN element keeps its x, an infinite one turns NaN
        proj = PC.no_step(f"nonfinite-g-{v}")
        assert np.array_equal(res[("g", "l2")][others], proj[others])
        assert (res[("g", "l2")][at] == proj[at]) if v == "nan" else np.isnan(res[("g", "l2")][at])
        # x, x0
        for rule in PC.RULES:
            assert np.isnan(res[("x", rule)][at]) == (v == "nan" or rule == "l2")
            assert np.isnan(res[("x0", rule)][at]) == (v == "nan" or rule == "l2")
        if v != "nan":
            s = 1.0 if v == "+inf" else -1.0
            assert res[("x", "linf")][at] == np.float32(base.x0[at] + np.float32(s * base.eps))
            assert res[("x0", "linf")][at] == s * np.inf
            for who in ("x", "x0"):                                # an infinite delta: factor 0, the row returns to x0
                row = res[(who, "l2")][at[0]]
                keep = np.arange(base.cols) != at[1]
                assert np.array_equal(row[keep], base.x0[at[0]][keep])


@pytest.mark.parametrize("edge", list(PC.SUMSQ_EDGES))
def test_handed_in_sum_of_squares_edges(lib, edge):
    """0, NaN and +inf: no step (alpha / inf = 0 and the gradient is finite): the projection alone, bit for bit"""
    c = PC.case("nonfinite-base")
    out = PC.host_step(c, "l2", sumsq=PC.SUMSQ_EDGES[edge])
    assert np.array_equal(out.view(np.uint32), PC.no_step("nonfinite-base").view(np.uint32))
    PC.check("host " + edge, c, "l2", out, PC.oracle(c, "l2", sumsq=PC.SUMSQ_EDGES[edge], K=PC.K_NORMED))


def test_tiny_sum_of_squares(lib):
    """a sum below FLT_MIN, which a float32 holds as a denormal of a few bits: the root is taken in double (csrc/gsr_pgd.h);
    a norm below FLT_MIN is no step"""
    b = PC.case("grad-1e-15")
    c = PC.Case("grad-1e-23-normed", b.x, (b.g.astype(np.float64) * 1e-8).astype(np.float32), b.x0, b.alpha, b.eps)
    assert 0 < PC.true_sumsq(c) < 1e-40
    PC.check("host", c, "l2", PC.host_step(c, "l2"), PC.oracle(c, "l2", K=PC.K_NORMED))
    assert np.array_equal(PC.host_step(c, "l2", sumsq=1e-80), PC.host_step(c, "l2", g=np.zeros_like(c.g)))


def test_handed_in_sum_of_squares_is_used(lib):
    c = PC.case("sweep-c45-r69")
    ss = PC.true_sumsq(c)
    assert np.array_equal(PC.host_step(c, "l2", sumsq=ss), PC.host_step(c, "l2"))
    PC.check("host 4x sum", c, "l2", PC.host_step(c, "l2", sumsq=4 * ss), PC.oracle(c, "l2", sumsq=4 * ss, K=PC.K_NORMED))
    assert PC.worst_ratio(PC.host_step(c, "l2", sumsq=4 * ss), PC.oracle(c, "l2", K=PC.K_NORMED)) > 1.0


def test_the_oracle_notices_small_faults():
    """the tolerance is tight enough to see a dropped 1e-7 and a row 2e-6 too long; a row on the threshold that was clipped
    lies inside the either-branch band, and its bits tell"""
    for name, scale in (("eps1e-3", 1.0 + 1e-7 / 4e-3),    # eps / nrm for eps / (nrm + 1e-7): 2.5e-5 at least where nrm <= 4 eps
                        ("sweep-c5-r65", 1.0 + 2e-6)):     # any row 2e-6 too long
        c = PC.case(name)
        ref = PC.oracle(c, "l2", K=PC.K_NORMED)
        good = PC.host_step(c, "l2")
        assert PC.worst_ratio(good, ref) <= 1.0
        k = np.nonzero(ref.clipped & ~ref.band)[0][0]
        bad = good.copy()
        bad[k] = (c.x0[k] + (good[k].astype(np.float64) - c.x0[k]) * scale).astype(np.float32)
        assert PC.worst_ratio(bad, ref) > 1.0, name
    t = PC.case("threshold8-c3")
    tref = PC.oracle(t, "l2", K=PC.K_NORMED)
    out = PC.host_step(t, "l2").copy()
    f = np.float32(0.625) / (np.float32(0.625) + np.float32(1e-7))
    assert f < 1 and np.float32(5) / (np.float32(5) + np.float32(1e-7)) == 1                  # why the eighth-size cases exist
    out[0] = t.x0[0] + (t.x[0] - t.x0[0]) * f                                                 # the row on the threshold, clipped
    assert PC.worst_ratio(out, tref) <= 1.0                                                   # inside the band: only the bits tell
    with pytest.raises(AssertionError):
        PC.check("mutant", t, "l2", out, tref, quiet=True)


def test_fuzz_against_oracle(lib):
    worst, plain = {r: 0.0 for r in PC.RULES}, 0
    for seed in range(200):
        c = PC.fuzz_case(seed)
        for rule in PC.RULES:
            ref = PC.oracle(c, rule, K=PC.K_NORMED)
            got = PC.host_step(c, rule)
            worst[rule] = max(worst[rule], PC.check("host fuzz", c, rule, got, ref, quiet=True, norm_error=True))
            plain += PC.property_excess(got, ref) > 0
    print("pgd host fuzz (200 seeds), worst error / bound:", {k: round(v, 3) for k, v in worst.items()},
          f"; seeds past the ball's allowance without the norm's error: {plain}")


def test_capped_grid_case_on_the_host(lib):
    c = PC.case(PC.CAPPED)
    assert PC.sumsq_blocks(c.n) == 1024 and c.n > 4 * 256 * 1024 and c.n % 4 == 3
    assert not c.g.reshape(-1)[:4 * 256 * 1024].any() and c.g.reshape(-1)[-3:].all()
    ref = PC.oracle(c, "l2", K=PC.K_NORMED)
    PC.check("host", c, "l2", PC.host_step(c, "l2"), ref)
    assert PC.worst_ratio(PC.no_step(PC.CAPPED), ref) > 1.0      # a skipped second trip would show


def test_launch_arithmetic(lib):
    for cols in range(1, PC.MAX_COLS + 1):
        assert lib.ph_rows_per_wave(cols) == PC.rows_per_wave(cols) == (64 if cols <= 24 else 32)
        assert PC.rows_per_wave(cols) * cols <= 64 * 24                          # the wave's deltas fit the LDS buffer
    for n in (1, 4095, 4096, 4097, 8193, 4096 * 1024, 4096 * 1024 + 1, PC.CAPPED_N, 1 << 33):
        assert lib.ph_sumsq_blocks(n) == PC.sumsq_blocks(n) == min(-(-n // 4096), 1024)
    assert PC.chain_length(4096) == 16 and PC.chain_length(4097) == 9 and PC.chain_length(PC.CAPPED_N) == 21
    r = np.random.default_rng(5)
    for trial in range(300):
        n = int(r.integers(1, PC.MAX_TENSORS + 1))
        blocks = r.integers(0, 4, n) * r.integers(0, 2, n)                       # many tensors without rows, anywhere
        first = np.zeros(PC.MAX_TENSORS + 1, np.uint32)
        first[1:n + 1] = np.cumsum(blocks)
        first[n:] = first[n]
        for b in range(int(first[n])):
            t = lib.ph_tensor_of_block(first.ctypes.data, n, b)
            assert first[t] <= b < first[t + 1] and blocks[t] > 0, (trial, first, b, t)


def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "pgd_host_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DPGD_MAIN", "-I", PC.CSRC, PC.SRC, "-o", exe], check=True)
    runs = [(name, rule, None) for name in PC.NAMES for rule in PC.case(name).rules]
    runs += [("nonfinite-base", "l2", v) for v in PC.SUMSQ_EDGES.values()]
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        f.write(np.array([len(runs)], np.int32).tobytes())
        for name, rule, ss in runs:
            c = PC.case(name)
            f.write(np.array([c.rows, c.cols, rule == "l2", ss is not None], np.int32).tobytes())
            f.write(np.array([c.alpha, c.eps], np.float32).tobytes())
            f.write(np.array([0.0 if ss is None else ss], np.float64).tobytes())
            f.write(c.x.tobytes() + c.g.tobytes() + c.x0.tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"cases {len(runs)} lookup 24"
    for k, (name, rule, ss) in enumerate(runs):   # the same answers as the library the other tests load
        c = PC.case(name)
        want = f"case {k} rows {c.rows} cols {c.cols} l2 {int(rule == 'l2')} hash {PC.fnv1a(PC.host_step(c, rule, sumsq=ss))}"
        assert lines[k] == want, (name, rule)


# ---- the CPU branch of gsplat_attack.pgd: the tensor formulation -------------------------------------------------------------
def _formulation(c, rule):
    from gsplat_attack import pgd
    x = torch.from_numpy(c.x.copy())
    (pgd.l2_step_ if rule == "l2" else pgd.linf_step_)(x, torch.from_numpy(c.g.copy()), c.alpha, c.eps, torch.from_numpy(c.x0.copy()))
    return x.numpy()


@pytest.mark.parametrize("group", ["sweep", "threshold", "other", "mass", "nonfinite"])
def test_cpu_branch_matches_oracle(group):
    """the formulation the contract is read from.  Its gradient norm is a float32 sum too: the same K; cases whose step may be
    lost may lose it here as well (the zero-gradient result of the formulation itself)"""
    names = dict(sweep=PC.SWEEP, threshold=PC.THRESHOLD, other=PC.OTHER, mass=PC.MASS, nonfinite=PC.NONFINITE)[group]
    worst = {r: 0.0 for r in PC.RULES}
    for name in names:
        c = PC.case(name)
        for rule in c.rules:
            lost = None
            if c.either:
                z = PC.Case(name, c.x, np.zeros_like(c.g), c.x0, c.alpha, c.eps)
                lost = _formulation(z, rule)
            worst[rule] = max(worst[rule], PC.check("cpu branch", c, rule, _formulation(c, rule), no_step=lost, quiet=True))
    print(f"pgd cpu branch {group}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


def test_host_build_and_cpu_branch_agree_bit_for_bit_under_linf():
    for name in PC.SWEEP[::5] + PC.OTHER + PC.NONFINITE:
        c = PC.case(name)
        a, b = PC.host_step(c, "linf"), _formulation(c, "linf")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
            a[~np.isnan(a)], b[~np.isnan(b)])), name

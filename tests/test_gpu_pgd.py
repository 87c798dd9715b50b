"""The projected-gradient step on the HIP path (csrc/gsr_pgd.h, csrc/gsr_pgd.hip.h) against the float64 oracle and the derived
tolerance of tests/pgd_cases.py: every named case through gsr_pgd_step (base pointers shifted off the 16-byte boundary one by
one, sentinels around x, grad and x0 untouched, a repeat bit-equal), gsr_pgd_step_normed and gsr_pgd_step_multi (per-tensor
alpha / eps, tensors without rows, sums handed in for some); the refusals; and the routes of gsplat_attack.pgd."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import pgd_cases as PC

pytestmark = pytest.mark.gpu

PAD, SENT = 64, -7.25
GSR_ERR_INVALID = 1


@functools.lru_cache(maxsize=None)
def _lib():
    import diff_gaussian_rasterization as D
    return D._load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err():
    import diff_gaussian_rasterization as D
    return D._err(_lib())


class Guarded:
    """a device copy of `a` that starts `shift` floats past a 16-byte boundary, with PAD sentinel floats on either side"""

    def __init__(self, a: np.ndarray, shift: int = 0):
        self.n, self.o = a.size, PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 4,), SENT, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.o:self.o + self.n] = torch.from_numpy(np.array(a, np.float32).reshape(-1))   # a copy: the cases are read-only
        self.ptr = self.buf.data_ptr() + 4 * self.o
        assert self.ptr % 16 == 4 * shift

    def get(self) -> np.ndarray:
        h = self.buf.cpu().numpy()
        assert (h[:self.o] == SENT).all() and (h[self.o + self.n:] == SENT).all(), "floats around the tensor were written"
        return h[self.o:self.o + self.n].copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def run_step(c, rule, shifts=(0, 0, 0), sumsq=None):
    """gsr_pgd_step, or gsr_pgd_step_normed when a sum of squares is handed in.  -> the new x [rows, cols]; asserts that nothing
    around x was written and that grad and x0 (and the floats around them) are bit for bit what they were"""
    x, g, x0 = Guarded(c.x, shifts[0]), Guarded(c.g, shifts[1]), Guarded(c.x0, shifts[2])
    if sumsq is None:
        rc = _lib().gsr_pgd_step(x.ptr, g.ptr, x0.ptr, c.rows, c.cols, c.alpha, c.eps, 1 if rule == "l2" else 0, _stream())
    else:
        ss = torch.tensor([sumsq], dtype=torch.float64, device="cuda")
        rc = _lib().gsr_pgd_step_normed(x.ptr, g.ptr, x0.ptr, c.rows, c.cols, c.alpha, c.eps, ss.data_ptr(), _stream())
    assert rc == 0, _err()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(g.get()), _bits(c.g)) and np.array_equal(_bits(x0.get()), _bits(c.x0)), "grad or x0 was written"
    return x.get().reshape(c.rows, c.cols)


def _shifts_of(name):
    i = (PC.NAMES.index(name) * 7 + 1) % 64 if name in PC.CASES else 27
    return (i % 4, (i // 4) % 4, (i // 16) % 4)


def _step_case(name, worst):
    """one case through gsr_pgd_step on the 16-byte path (no shift) and at the case's own shifts, both rules"""
    c = PC.case(name)
    for rule in c.rules:
        lost = PC.no_step(name) if c.either else None
        for shifts in ((0, 0, 0), _shifts_of(name)):
            got = run_step(c, rule, shifts)
            w = PC.check(f"step {shifts}", c, rule, got, no_step=lost, quiet=True)
            worst[rule] = max(worst.get(rule, 0.0), w)
            if rule == "linf":      # single IEEE operations: the host build's bits
                assert np.array_equal(_bits(got), _bits(PC.host_step(c, rule))), (name, shifts)
            elif not c.g.any():     # zero gradient: the same
                assert np.array_equal(_bits(got), _bits(PC.no_step(name))), (name, shifts)
        assert np.array_equal(_bits(run_step(c, rule, shifts)), _bits(got)), (name, rule, "a second run differs")


@pytest.mark.parametrize("cols", range(1, PC.MAX_COLS + 1))
def test_step_sweep(cols):
    worst = {}
    for rows in PC.sweep_rows(cols):
        _step_case(f"sweep-c{cols}-r{rows}", worst)
    print(f"pgd device step sweep cols {cols}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name", PC.THRESHOLD + PC.OTHER + PC.MASS + PC.NONFINITE)
def test_step_named_case(name):
    worst = {}
    _step_case(name, worst)
    print(f"pgd device step {name}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name", ["sweep-c45-r69", "sweep-c3-r133", "sweep-c16-r64", "sweep-c25-r32"])
def test_step_at_every_combination_of_shifts(name):
    """x, grad and x0 each 0..3 floats past a 16-byte boundary, independently: the 16-byte path needs all three of the step
    kernel's (and grad's alone in the sum of squares), every other combination falls back.  Per element the arithmetic is the
    same: L-inf gives the same bits everywhere, L2 the same bits wherever grad's shift -- the order of the sum -- is the same."""
    c = PC.case(name)
    worst = {}
    for rule in PC.RULES:
        first = {}
        for i in range(64):
            shifts = (i % 4, (i // 4) % 4, (i // 16) % 4)
            got = run_step(c, rule, shifts)
            worst[rule] = max(worst.get(rule, 0.0), PC.check(f"step {shifts}", c, rule, got, quiet=True))
            key = 0 if rule == "linf" else (shifts[1] == 0)
            assert np.array_equal(_bits(got), _bits(first.setdefault(key, got))), (name, rule, shifts)
    print(f"pgd device step all shifts {name}: worst error / bound", {k: round(v, 3) for k, v in worst.items()})


def test_step_capped_grid():
    """n > 4 Mi floats: k_pgd_sumsq's grid is capped and its loop takes a second trip, where all of this gradient lies"""
    c = PC.case(PC.CAPPED)
    ref = PC.oracle(c, "l2")
    for shifts in ((0, 0, 0), (0, 1, 0)):          # the 16-byte loop and its tail; the 4-byte loop
        PC.check(f"step {shifts}", c, "l2", run_step(c, "l2", shifts), ref)


# ---- gsr_pgd_step_normed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["sweep", "threshold", "other", "mass", "nonfinite"])
def test_normed_matches_oracle(group):
    """the oracle's float64 sum of squares handed in on the device: K = 4.  Reported: how many results are bit for bit the host
    build's, which takes the same sum through the same header."""
    names = dict(sweep=PC.SWEEP, threshold=PC.THRESHOLD, other=PC.OTHER, mass=PC.MASS, nonfinite=PC.NONFINITE)[group]
    worst, same, n = 0.0, 0, 0
    for name in names:
        c = PC.case(name)
        if "l2" not in c.rules:
            continue
        ss = PC.true_sumsq(c)
        got = run_step(c, "l2", _shifts_of(name), sumsq=ss)
        ref = PC.oracle(c, "l2", sumsq=ss, K=PC.K_NORMED)
        worst = max(worst, PC.check("normed", c, "l2", got, ref, no_step=PC.no_step(name) if c.either else None, quiet=True))
        n, same = n + 1, same + bool(np.array_equal(_bits(got), _bits(PC.host_step(c, "l2", sumsq=ss))))
    print(f"pgd device normed {group}: worst error / bound {worst:.3f}; bit-equal to the host build in {same} of {n} cases")


@pytest.mark.parametrize("edge", list(PC.SUMSQ_EDGES))
def test_normed_sum_of_squares_edges(edge):
    """0, NaN, +inf: no step; the projection alone, bit for bit the host build's"""
    c = PC.case("nonfinite-base")
    got = run_step(c, "l2", (0, 0, 0), sumsq=PC.SUMSQ_EDGES[edge])
    PC.check("normed " + edge, c, "l2", got, PC.oracle(c, "l2", sumsq=PC.SUMSQ_EDGES[edge], K=PC.K_NORMED))
    assert np.array_equal(_bits(got), _bits(PC.no_step("nonfinite-base")))


def test_normed_tiny_sum_of_squares():
    """a sum below FLT_MIN, which a float32 holds as a denormal of a few bits: the root is taken in double (csrc/gsr_pgd.h)"""
    b = PC.case("grad-1e-15")
    c = PC.Case("grad-1e-23-normed", b.x, (b.g.astype(np.float64) * 1e-8).astype(np.float32), b.x0, b.alpha, b.eps)
    ss = PC.true_sumsq(c)
    assert 0 < ss < 1e-40
    PC.check("normed", c, "l2", run_step(c, "l2", (0, 0, 0), sumsq=ss), PC.oracle(c, "l2", sumsq=ss, K=PC.K_NORMED))


# ---- gsr_pgd_step_multi ----------------------------------------------------------------------------------------------------
def _packs(rule):
    """the named cases in groups of 7 plus one tensor without rows -- first, in the middle, last in turn -- each with an alpha
    and an eps of its own"""
    names = [n for n in PC.NAMES if rule in PC.case(n).rules]
    order = np.random.default_rng(3).permutation(len(names))         # mix the groups: eps = 5 beside eps = 1e-6
    names = [names[i] for i in order]
    packs = []
    for k in range(0, len(names), 7):
        pack = []
        for t, name in enumerate(names[k:k + 7]):
            b = PC.case(name)
            scaled = PC.Case(name, b.x, b.g, b.x0, b.alpha * (1 + 0.25 * t), b.eps * (1 + 0.125 * t), rules=b.rules, either=b.either)
            pack.append(scaled if name.startswith("sweep-") else b)   # the others keep the parameters their point depends on
        pack.insert((0, len(pack) // 2, len(pack))[len(packs) % 3], None)
        packs.append(pack)
    return packs


@pytest.mark.parametrize("rule", PC.RULES)
def test_multi_equals_the_per_tensor_calls_and_the_oracle(rule):
    lib, l2 = _lib(), rule == "l2"
    worst, ntens = 0.0, 0
    for p, pack in enumerate(_packs(rule)):
        n = len(pack)
        bufs, sums, dev_ss = [], [], []
        for t, c in enumerate(pack):
            sh = ((p + t) % 4, (p + 2 * t) % 4, (p // 4 + t) % 4)
            bufs.append(None if c is None else (Guarded(c.x, sh[0]), Guarded(c.g, sh[1]), Guarded(c.x0, sh[2]), sh))
            sums.append(PC.true_sumsq(c) if (c is not None and l2 and t % 2 == 1) else None)   # handed in for every other tensor
            dev_ss.append(None if sums[t] is None else torch.tensor([sums[t]], dtype=torch.float64, device="cuda"))
        arr = lambda k: (ctypes.c_void_p * n)(*[None if b is None else b[k].ptr for b in bufs])   # noqa: E731
        ssp = (ctypes.c_void_p * n)(*[None if s is None else s.data_ptr() for s in dev_ss])
        rc = lib.gsr_pgd_step_multi(n, arr(0), arr(1), arr(2), (ctypes.c_int64 * n)(*[0 if c is None else c.rows for c in pack]),
                                    (ctypes.c_int32 * n)(*[7 if c is None else c.cols for c in pack]),
                                    (ctypes.c_float * n)(*[0.5 if c is None else c.alpha for c in pack]),
                                    (ctypes.c_float * n)(*[0.5 if c is None else c.eps for c in pack]), 1 if l2 else 0, ssp, _stream())
        assert rc == 0, _err()
        torch.cuda.synchronize()
        for t, c in enumerate(pack):
            if c is None:
                continue
            xg, gg, x0g, sh = bufs[t]
            got = xg.get().reshape(c.rows, c.cols)
            assert np.array_equal(_bits(gg.get()), _bits(c.g)) and np.array_equal(_bits(x0g.get()), _bits(c.x0))
            alone = run_step(c, rule, sh, sumsq=sums[t])
            assert np.array_equal(_bits(got), _bits(alone)), (p, t, c.name, "multi differs from the per-tensor call")
            ref = PC.oracle(c, rule, sumsq=sums[t], K=PC.K_NORMED if sums[t] is not None else None)
            lost = PC.host_step(c, rule, g=np.zeros_like(c.g)) if c.either else None
            worst = max(worst, PC.check(f"multi pack {p} tensor {t}", c, rule, got, ref, no_step=lost, quiet=True))
            ntens += 1
    print(f"pgd device multi {rule}: {ntens} tensors, worst error / bound {worst:.3f}")


def test_multi_of_eight_tensors_without_rows_and_with_them():
    """eight at once; and only tensors without rows: nothing is launched"""
    lib = _lib()
    n = 8
    null = (ctypes.c_void_p * n)()
    rc = lib.gsr_pgd_step_multi(n, null, null, null, (ctypes.c_int64 * n)(), (ctypes.c_int32 * n)(*([3] * n)), (ctypes.c_float * n)(),
                                (ctypes.c_float * n)(), 1, None, _stream())
    assert rc == 0, _err()
    cases = [PC.case(f"sweep-c{cols}-r{PC.sweep_rows(cols)[3]}") for cols in (1, 2, 16, 24, 25, 47, 48, 45)]
    for l2 in (0, 1):
        bufs = [(Guarded(c.x), Guarded(c.g), Guarded(c.x0)) for c in cases]
        arr = lambda k: (ctypes.c_void_p * n)(*[b[k].ptr for b in bufs])   # noqa: E731
        rc = lib.gsr_pgd_step_multi(n, arr(0), arr(1), arr(2), (ctypes.c_int64 * n)(*[c.rows for c in cases]),
                                    (ctypes.c_int32 * n)(*[c.cols for c in cases]), (ctypes.c_float * n)(*[c.alpha for c in cases]),
                                    (ctypes.c_float * n)(*[c.eps for c in cases]), l2, None, _stream())
        assert rc == 0, _err()
        torch.cuda.synchronize()
        for c, b in zip(cases, bufs):
            rule = "l2" if l2 else "linf"
            got = b[0].get().reshape(c.rows, c.cols)
            PC.check("multi of 8", c, rule, got, quiet=True)
            assert np.array_equal(_bits(got), _bits(run_step(c, rule)))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_alone():
    lib = _lib()
    c = PC.case("sweep-c3-r65")
    x, g, x0 = Guarded(c.x), Guarded(c.g), Guarded(c.x0)
    ss = torch.tensor([1.0], dtype=torch.float64, device="cuda")
    one = lambda ptr: (ctypes.c_void_p * 1)(ptr)   # noqa: E731
    i64, i32, f32 = (lambda v: (ctypes.c_int64 * 1)(v)), (lambda v: (ctypes.c_int32 * 1)(v)), (lambda v: (ctypes.c_float * 1)(v))   # noqa: E731
    bad = []
    for rows, cols in ((c.rows, 0), (c.rows, 49), (-1, 3), (c.rows, -3)):
        bad.append((f"step rows {rows} cols {cols}", lambda r=rows, k=cols: lib.gsr_pgd_step(x.ptr, g.ptr, x0.ptr, r, k, 0.5, 0.8, 1, _stream())))
        bad.append((f"normed rows {rows} cols {cols}",
                    lambda r=rows, k=cols: lib.gsr_pgd_step_normed(x.ptr, g.ptr, x0.ptr, r, k, 0.5, 0.8, ss.data_ptr(), _stream())))
        bad.append((f"multi rows {rows} cols {cols}",
                    lambda r=rows, k=cols: lib.gsr_pgd_step_multi(1, one(x.ptr), one(g.ptr), one(x0.ptr), i64(r), i32(k), f32(0.5), f32(0.8), 1,
                                                                  None, _stream())))
    for k in range(3):
        ptrs = [x.ptr, g.ptr, x0.ptr]
        ptrs[k] = None
        for l2 in (0, 1):
            bad.append((f"step null {k}", lambda p=tuple(ptrs), m=l2: lib.gsr_pgd_step(*p, c.rows, 3, 0.5, 0.8, m, _stream())))
            bad.append((f"multi null {k}", lambda p=tuple(ptrs), m=l2: lib.gsr_pgd_step_multi(1, one(p[0]), one(p[1]), one(p[2]), i64(c.rows), i32(3),
                                                                                           f32(0.5), f32(0.8), m, None, _stream())))
        bad.append((f"normed null {k}", lambda p=tuple(ptrs): lib.gsr_pgd_step_normed(*p, c.rows, 3, 0.5, 0.8, ss.data_ptr(), _stream())))
    bad.append(("normed null sum", lambda: lib.gsr_pgd_step_normed(x.ptr, g.ptr, x0.ptr, c.rows, 3, 0.5, 0.8, None, _stream())))
    nine = (ctypes.c_void_p * 9)(*([x.ptr] * 9))
    bad.append(("multi n = 9", lambda: lib.gsr_pgd_step_multi(9, nine, nine, nine, (ctypes.c_int64 * 9)(*([1] * 9)), (ctypes.c_int32 * 9)(*([3] * 9)),
                                                              (ctypes.c_float * 9)(), (ctypes.c_float * 9)(), 0, None, _stream())))
    bad.append(("multi n = -1", lambda: lib.gsr_pgd_step_multi(-1, nine, nine, nine, (ctypes.c_int64 * 9)(), (ctypes.c_int32 * 9)(),
                                                               (ctypes.c_float * 9)(), (ctypes.c_float * 9)(), 0, None, _stream())))
    bad.append(("multi null arrays", lambda: lib.gsr_pgd_step_multi(1, None, None, None, None, None, None, None, 0, None, _stream())))
    for what, call in bad:
        assert call() == GSR_ERR_INVALID, what
        assert "gsr_pgd_step" in _err(), what
    torch.cuda.synchronize()
    assert np.array_equal(_bits(x.get()), _bits(c.x)) and np.array_equal(_bits(g.get()), _bits(c.g)) and np.array_equal(_bits(x0.get()), _bits(c.x0))
    # no rows: accepted, nothing done, null pointers allowed
    assert lib.gsr_pgd_step(None, None, None, 0, 3, 0.5, 0.8, 1, _stream()) == 0
    assert lib.gsr_pgd_step_normed(None, None, None, 0, 3, 0.5, 0.8, None, _stream()) == 0


# ---- the binding's routes ----------------------------------------------------------------------------------------------------
def _route(x, grad, x0, rule, c, takes_kernel, sumsq=None):
    """x stepped in place through gsplat_attack.pgd; -> its values.  The kernel route warns nothing; the tensor-op route warns
    once"""
    from gsplat_attack import pgd
    step = pgd.l2_step_ if rule == "l2" else pgd.linf_step_
    pgd._WARNED.clear()
    v = x._version
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        step(x, grad, c.alpha, c.eps, x0)
    torch.cuda.synchronize()
    ours = [m for m in w if "gsr_pgd_step" in str(m.message)]
    assert len(ours) == (0 if takes_kernel else 1), [str(m.message) for m in w]
    assert x._version > v
    return x.detach().cpu().double().numpy()


@pytest.mark.parametrize("rule", PC.RULES)
def test_binding_routes(rule):
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731
    # the kernel: a 1-D tensor (one column), [rows, 15, 3], a non-contiguous or float64 grad, a float16 x0
    c1 = PC.case("sweep-c1-r133")
    PC.check("route 1-D", c1, rule, _route(dev(c1.x).reshape(-1), dev(c1.g).reshape(-1), dev(c1.x0).reshape(-1), rule, c1, True))
    c = PC.case("sweep-c45-r69")
    sh = (c.rows, 15, 3)
    kernel = np.ascontiguousarray(run_step(c, rule))
    got = _route(dev(c.x).reshape(sh), dev(c.g).reshape(sh), dev(c.x0).reshape(sh), rule, c, True)
    PC.check("route [rows,15,3]", c, rule, got)
    assert np.array_equal(_bits(got), _bits(kernel))
    wide = torch.zeros(c.rows, 2 * c.cols, device="cuda")
    wide[:, ::2] = dev(c.g)
    assert not wide[:, ::2].is_contiguous()
    assert np.array_equal(_bits(_route(dev(c.x), wide[:, ::2], dev(c.x0), rule, c, True)), _bits(kernel))
    assert np.array_equal(_bits(_route(dev(c.x), dev(c.g).double(), dev(c.x0), rule, c, True)), _bits(kernel))
    half = PC.Case("half-x0", c.x, c.g, c.x0.astype(np.float16).astype(np.float32), c.alpha, c.eps)
    PC.check("route float16 x0", half, rule, _route(dev(c.x), dev(c.g), dev(c.x0).half(), rule, half, True))
    # the tensor formulation, with one warning: a non-contiguous x, a float64 x, 49 columns
    xw = torch.zeros(c.rows, 2 * c.cols, device="cuda")
    xw[:, ::2] = dev(c.x)
    PC.check("route strided x", c, rule, _route(xw[:, ::2], dev(c.g), dev(c.x0), rule, c, False))
    PC.check("route float64 x", c, rule, _route(dev(c.x).double(), dev(c.g).double(), dev(c.x0).double(), rule, c, False))
    r = np.random.default_rng(49)
    x49, x0_49 = PC._spread(r, 70, 49, 0.8)
    c49 = PC.Case("cols49", x49, r.standard_normal((70, 49)) * 3, x0_49, 0.5, 0.8)
    PC.check("route 49 columns", c49, rule, _route(dev(c49.x), dev(c49.g), dev(c49.x0), rule, c49, False), PC.oracle(c49, rule))


@pytest.mark.parametrize("rule", PC.RULES)
def test_binding_multi_step_route(rule):
    from gsplat_attack import pgd
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731
    c1, c = PC.case("sweep-c1-r133"), PC.case("sweep-c45-r69")
    xs = [dev(c1.x).reshape(-1), dev(c.x).reshape(c.rows, 15, 3)]
    items = [(xs[0], dev(c1.g).reshape(-1), dev(c1.x0).reshape(-1), None), (xs[1], dev(c.g).reshape(c.rows, 15, 3), dev(c.x0).reshape(c.rows, 15, 3), None)]
    vers = [t._version for t in xs]
    assert pgd.multi_step_(items, c.alpha, c.eps, rule == "l2")
    torch.cuda.synchronize()
    for t, cc, v in zip(xs, (c1, c), vers):
        assert t._version > v
        PC.check("route multi_step_", cc, rule, t.cpu().numpy())
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(run_step(cc, rule)))

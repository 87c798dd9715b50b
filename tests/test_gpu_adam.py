"""The fused Adam step on the HIP path (csrc/gsr_adam.h, csrc/gsr_adam.hip.h): gsr_adam_step_multi BIT FOR BIT the host build of
the same header on every case of tests/adam_cases.py (no tolerance: the project's rule for GSR_FP_STRICT sources; a NaN is a
NaN whatever its payload), with sentinels around every tensor untouched and the gradient unwritten; rows left out of a mask
or a range bit for bit their inputs, guard values included; the refusals; two streams; and the optimiser's route."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import adam_cases as AC

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
        self.n, self.o, self.shape = a.size, PAD + shift, a.shape
        self.buf = torch.full((self.n + 2 * PAD + 4,), SENT, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.o:self.o + self.n] = torch.from_numpy(np.array(a, np.float32).reshape(-1))   # a copy: the cases are read-only
        self.ptr = self.buf.data_ptr() + 4 * self.o
        assert self.ptr % 16 == 4 * shift

    def get(self) -> np.ndarray:
        h = self.buf.cpu().numpy()
        assert (h[:self.o] == SENT).all() and (h[self.o + self.n:] == SENT).all(), "floats around the tensor were written"
        return h[self.o:self.o + self.n].copy().reshape(self.shape)


def _same(a, b) -> bool:
    """the same bits, or a NaN on both sides (the payload of a generated NaN is the machine's)"""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def device_call(c, bufs, mask_dev=None, stream=None):
    n = c.n
    arr = lambda k: (ctypes.c_void_p * n)(*[b[k].ptr if b[k].n else None for b in bufs])   # noqa: E731
    f32 = lambda v: (ctypes.c_float * n)(*v)   # noqa: E731
    return _lib().gsr_adam_step_multi(n, arr(0), arr(1), arr(2), arr(3), (ctypes.c_int64 * n)(*[four[0].shape[0] for four in c.tensors]),
                                      (ctypes.c_int32 * n)(*[four[0].shape[1] for four in c.tensors]), f32(c.lr), f32(c.b1), f32(c.b2),
                                      f32(c.eps), c.step, None if mask_dev is None else mask_dev.data_ptr(),
                                      *((0, -1) if c.rows is None else c.rows), stream or _stream())


def device_run(c, shift=None):
    """-> [(x, m, v), ...] after gsr_adam_step_multi; asserts that nothing around the tensors and no gradient was written"""
    shift = c.shift if shift is None else shift
    bufs = [[Guarded(a, s) for a in four] for four, s in zip(c.tensors, shift)]
    mask_dev = None if c.mask is None else torch.from_numpy(c.mask.copy()).cuda()
    rc = device_call(c, bufs, mask_dev)
    assert rc == 0, _err()
    torch.cuda.synchronize()
    out = []
    for b, four in zip(bufs, c.tensors):
        assert _same(b[1].get(), four[1]), "the gradient was written"
        out.append((b[0].get(), b[2].get(), b[3].get()))
    return out


def assert_host_bits(c, got, label=""):
    for t, (g3, h3) in enumerate(zip(got, AC.host_run(c))):
        for what, a, b in zip("xmv", g3, h3):
            assert _same(a, b), f"{c.name} {label} tensor {t} {what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} elements differ from the host build"


@pytest.mark.parametrize("cols", AC.SWEEP_COLS)
def test_sweep_is_bit_equal_to_the_host_build(cols):
    """every sweep case on the 16-byte path and with the tensor one float off the boundary (the 4-byte path)"""
    for rows in AC.SWEEP_ROWS:
        for t in AC.SWEEP_T:
            c = AC.case(AC.sweep_name(cols, rows, t))
            for shift in ([0], [1]):
                got = device_run(c, shift)
                assert_host_bits(c, got, f"shift {shift}")
            assert AC.moved_fraction(c, got) >= 0.99, c.name


@pytest.mark.parametrize("name", AC.PACKS + AC.OTHER + AC.NONFINITE)
def test_named_case_is_bit_equal_to_the_host_build(name):
    c = AC.case(name)
    got = device_run(c)
    assert_host_bits(c, got)
    if name not in AC.NONFINITE:
        AC.check("device", c, got)                            # and so within the derived bounds of torch.optim.Adam
    else:
        for a, r in zip(got[0], AC.oracle(c, torch.float32)[0]):
            assert np.array_equal(AC.classes(a), AC.classes(r)), name
    assert all(_same(a, b) for g3, h3 in zip(device_run(c), got) for a, b in zip(g3, h3)), "a second run differs"


def test_gradient_beyond_the_root_of_flt_max_is_bit_equal_to_the_host_build():
    c = AC.beyond_root_case()
    got = device_run(c)
    assert_host_bits(c, got)
    assert np.isposinf(got[0][2][AC.NONFINITE_AT]) and got[0][0][AC.NONFINITE_AT] == c.tensors[0][0][AC.NONFINITE_AT]


def test_every_combination_of_shifts_of_one_tensor():
    """x, g, m, v each 0 or 1 float past a 16-byte boundary, independently: the 16-byte path needs all four"""
    c = AC.case("sweep-c45-r65-t10")
    x, g, m, v = c.tensors[0]
    host = AC.host_run(c)[0]
    for i in range(16):
        sh = [(i >> k) & 1 for k in range(4)]
        bufs = [[Guarded(a, s) for a, s in zip((x, g, m, v), sh)]]
        assert device_call(c, bufs) == 0, _err()
        torch.cuda.synchronize()
        for a, b in zip((bufs[0][0].get(), bufs[0][2].get(), bufs[0][3].get()), host):
            assert _same(a, b), sh


@pytest.mark.parametrize("name", AC.SELECT)
def test_mask_and_range(name):
    """bit for bit the host build; rows left out bit for bit their inputs -- also when they hold guard values (NaN gradients,
    sentinels in x, m, v), so that a stray read or write shows; live rows bit for bit the step without a selection"""
    c = AC.case(name)
    live = c.live(0)
    got = device_run(c)
    assert_host_bits(c, got)
    AC.check("device", c, got)
    full = device_run(c.without_selection())
    guarded = []
    for x, g, m, v in c.tensors:
        four = [a.copy() for a in (x, g, m, v)]
        four[0][~live], four[1][~live], four[2][~live], four[3][~live] = SENT, np.nan, 3e38, np.nan
        guarded.append(tuple(four))
    cg = AC.Call(name + "-guarded", guarded, c.lr, c.step, c.b1, c.b2, c.eps, mask=c.mask, rows=c.rows)
    got_g = device_run(cg)
    for t in range(c.n):
        for k, (a, b, ag) in enumerate(zip(got[t], full[t], got_g[t])):
            assert _same(a[live], b[live]) and _same(ag[live], b[live]), (name, t)
            assert _same(ag[~live], guarded[t][(0, 2, 3)[k]][~live]), (name, t, "a row left out was written")


def test_mask_of_bool_bytes_other_than_one_counts_as_live():
    c = AC.case("mask-alternating")
    loud = AC.Call("mask-255", c.tensors, c.lr, c.step, mask=c.mask * 255)
    for g3, h3 in zip(device_run(loud), device_run(c)):
        assert all(_same(a, b) for a, b in zip(g3, h3))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = _lib()
    c = AC.case("pack1")
    bufs = [[Guarded(a) for a in c.tensors[0]]]
    x, g, m, v = bufs[0]
    two = AC.Call("two", [c.tensors[0], AC.case("sweep-c3-r65-t1").tensors[0]], 1e-2, 1)
    bufs2 = [bufs[0], [Guarded(a) for a in two.tensors[1]]]
    mask = torch.ones(257, dtype=torch.uint8, device="cuda")
    one = lambda p: (ctypes.c_void_p * 1)(p)   # noqa: E731

    def call(n=1, rows=257, cols=3, lr=1e-2, b1=0.9, b2=0.999, eps=1e-15, step=1, mk=None, rb=0, re=-1, ptrs=None):
        p = ptrs or [x.ptr, g.ptr, m.ptr, v.ptr]
        return lib.gsr_adam_step_multi(n, one(p[0]), one(p[1]), one(p[2]), one(p[3]), (ctypes.c_int64 * 1)(rows), (ctypes.c_int32 * 1)(cols),
                                       (ctypes.c_float * 1)(lr), (ctypes.c_float * 1)(b1), (ctypes.c_float * 1)(b2), (ctypes.c_float * 1)(eps),
                                       step, mk, rb, re, _stream())
    bad = [dict(n=0), dict(n=9), dict(n=-1), dict(step=0), dict(step=-3), dict(cols=0), dict(cols=49), dict(rows=-1), dict(b1=1.0),
           dict(b1=-0.1), dict(b2=1.0), dict(b2=-1e-3), dict(eps=-1e-8), dict(lr=float("nan")), dict(lr=float("inf")), dict(eps=float("inf")),
           dict(b1=float("nan")), dict(b2=float("inf")), dict(rb=-1), dict(rb=5, re=4), dict(re=258), dict(rb=258, re=258),
           dict(mk=mask.data_ptr(), re=300)]
    for k in range(4):
        p = [x.ptr, g.ptr, m.ptr, v.ptr]
        p[k] = None
        bad.append(dict(ptrs=p))
    for kw in bad:
        assert call(**kw) == GSR_ERR_INVALID, kw
        assert "gsr_adam_step_multi" in _err(), kw
    nul = lambda: lib.gsr_adam_step_multi(1, None, None, None, None, None, None, None, None, None, None, 1, None, 0, -1, _stream())   # noqa: E731
    assert nul() == GSR_ERR_INVALID and "null" in _err()
    torch.cuda.synchronize()                                  # no refusal launched anything: every buffer keeps its input bits
    for b, a in zip((x, g, m, v), c.tensors[0]):
        assert _same(b.get(), a)
    # unequal row counts: fine without a selection, refused with a mask or a range
    assert device_call(two, bufs2) == 0, _err()
    torch.cuda.synchronize()
    stepped = [b.get() for b in (x, m, v)]
    for s, h in zip(stepped, AC.host_run(AC.Call("one", [c.tensors[0]], 1e-2, 1))[0]):
        assert _same(s, h)                                    # exactly one step of the good call
    for sel in (dict(mask=np.ones(257, np.uint8)), dict(rows=(0, 10))):
        refused = AC.Call("two-sel", two.tensors, 1e-2, 1, **sel)
        assert device_call(refused, bufs2, None if "mask" not in sel else mask) == GSR_ERR_INVALID
        assert "row" in _err()
    torch.cuda.synchronize()
    for b, s in zip((x, m, v), stepped):                      # nothing ran after the one good call
        assert _same(b.get(), s)
    assert _same(g.get(), c.tensors[0][1])
    # nothing to do: accepted, nothing launched
    assert call(rows=0, ptrs=[None] * 4) == 0 and call(rb=0, re=0) == 0 and call(rb=257, re=257) == 0
    torch.cuda.synchronize()
    for b, s in zip((x, m, v), stepped):
        assert _same(b.get(), s)


# ---- streams -------------------------------------------------------------------------------------------------------------------
def test_two_streams_stepping_two_models_give_the_sequential_bits():
    a, b = AC.case("pack7"), AC.case("mask-boundaries")
    seq = []
    for c in (a, b):
        outs = None
        bufs = [[Guarded(t) for t in four] for four in c.tensors]
        md = None if c.mask is None else torch.from_numpy(c.mask.copy()).cuda()
        for k in range(3):
            cc = AC.Call(c.name, c.tensors, c.lr, c.step + k, mask=c.mask)
            assert device_call(cc, bufs, md) == 0, _err()
        torch.cuda.synchronize()
        outs = [(f[0].get(), f[2].get(), f[3].get()) for f in bufs]
        seq.append(outs)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [[[Guarded(t) for t in four] for four in c.tensors] for c in (a, b)]
    masks = [None if c.mask is None else torch.from_numpy(c.mask.copy()).cuda() for c in (a, b)]
    torch.cuda.synchronize()
    for k in range(3):
        for i, c in enumerate((a, b)):
            cc = AC.Call(c.name, c.tensors, c.lr, c.step + k, mask=c.mask)
            assert device_call(cc, bufs[i], masks[i], ctypes.c_void_p(streams[i].cuda_stream)) == 0, _err()
    torch.cuda.synchronize()
    for i in range(2):
        for f, want in zip(bufs[i], seq[i]):
            for got, w in zip((f[0].get(), f[2].get(), f[3].get()), want):
                assert _same(got, w)


# ---- the binding and the optimiser ---------------------------------------------------------------------------------------------
def test_adam_step_binding_and_its_refusal_to_take_other_layouts():
    from diff_gaussian_rasterization import adam_ops
    assert adam_ops.available()
    c = AC.case("pack7")
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()   # noqa: E731
    shapes = [(257, 3), (257, 1, 3), (257, 15, 3), (257, 1), (257, 3), (257, 4), (257, 1, 16)]
    items = [tuple(dev(a).reshape(s) for a in four) for four, s in zip(c.tensors, shapes)]
    vers = [it[0]._version for it in items]
    assert adam_ops.adam_step_(items, c.step, c.lr, (c.b1[0], c.b2[0]), c.eps[0])
    torch.cuda.synchronize()
    for it, v, h in zip(items, vers, AC.host_run(c)):
        assert it[0]._version > v
        assert _same(it[0].cpu().numpy(), h[0]) and _same(it[2].cpu().numpy(), h[1]) and _same(it[3].cpu().numpy(), h[2])
    before = [t.clone() for t in items[0]]
    assert not adam_ops.adam_step_([tuple(t.double() for t in items[0])], 1, 1e-2, (0.9, 0.999), 1e-15)
    wide = torch.zeros(257, 6, device="cuda")
    assert not adam_ops.adam_step_([(wide[:, ::2], items[0][1], items[0][2], items[0][3])], 1, 1e-2, (0.9, 0.999), 1e-15)
    assert not adam_ops.adam_step_([tuple(t.cpu() for t in items[0])], 1, 1e-2, (0.9, 0.999), 1e-15)
    assert all(torch.equal(a, b) for a, b in zip(before, items[0]))


def test_optimizer_step_takes_the_kernel_increments_versions_and_a_saved_forward_notices():
    import warnings
    from gsplat_attack.optim import OptimizationParams
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device="cuda", n_views=1, width=64, height=64)
    model.training_setup(OptimizationParams())
    bg = torch.zeros(3, device="cuda")
    pipe = PipelineParams(skip_objects=True)
    out = render(cams[0], model, pipe, bg)["render"]
    out.sum().backward()
    before = [p.detach().clone() for p in model.parameters()]
    vers = [p._version for p in model.parameters()]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model.optimizer.step()
    torch.cuda.synchronize()
    assert not [m for m in w if "gsr_adam_step_multi" in str(m.message)]      # the kernel route warns nothing
    stepped = 0
    for name, p, b, v in zip(model.named_parameters(), model.parameters(), before, vers):
        if p.grad is None:
            assert torch.equal(p, b), name
            continue
        stepped += 1
        assert p._version > v and not torch.equal(p, b), name
    assert stepped >= 6 and model.optimizer.step_count == 1
    # the float64 oracle on one group: x_1 = x_0 - lr sign(g) wherever |g| is far above eps
    g = model._opacity.grad.double().cpu().numpy()
    dx = (model._opacity.detach().double().cpu().numpy() - before[5].double().cpu().numpy())
    big = np.abs(g) > 1e-9
    assert big.sum() > 100 and np.allclose(dx[big], -0.05 * np.sign(g[big]), rtol=1e-4, atol=1e-7)
    # a forward that saved the parameters and then sees them stepped: what a PGD step raises
    model.optimizer.zero_grad()
    out = render(cams[0], model, pipe, bg)["render"]
    model._features_dc.grad = torch.ones_like(model._features_dc)
    model.optimizer.step()
    with pytest.raises(RuntimeError, match="modified in place"):
        out.sum().backward()

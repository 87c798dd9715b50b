"""Adaptive density control on the HIP path (csrc/gsr_densify.h, csrc/gsr_densify.hip.h) against the host build of the same header
on every case of tests/densify_cases.py: BIT FOR BIT the counts, origin / kind, every copied element, every moment, the row
masks, the child scales and the statistics (no tolerance: a NaN is a NaN whatever its payload); child positions within the
derived bounds of tests/densify_cases.py (only expf, and with keyed normals logf, may differ) and, with the normals given, also
directly against the float64 oracle.  Sentinels around every destination untouched and every destination element written;
the sources unchanged; the refusals; two streams; run to run; the batch statistics; the model's route; a render after a
densify; a short refit with a densify schedule."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import densify_cases as DC

pytestmark = pytest.mark.gpu

PAD, SENT = 64, DC.SENT
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
    """a device buffer of `shape` float32 that starts `shift` floats past a 16-byte boundary, with PAD sentinel floats on either
    side; filled with `a`, or with the sentinel (a destination: every element must be written)"""

    def __init__(self, shape, a=None, shift: int = 0):
        self.shape, self.n, self.o = tuple(shape), int(np.prod(shape)), PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 4,), SENT, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        if a is not None:
            self.buf[self.o:self.o + self.n] = torch.from_numpy(np.array(a, np.float32).reshape(-1))
        self.ptr = (self.buf.data_ptr() + 4 * self.o) if self.n else None
        self.dest = a is None

    def get(self) -> np.ndarray:
        h = self.buf.cpu().numpy()
        assert (h[:self.o] == SENT).all() and (h[self.o + self.n:] == SENT).all(), "floats around the tensor were written"
        out = h[self.o:self.o + self.n].copy().reshape(self.shape)
        if self.dest:
            assert not (out.view(np.uint32) == np.float32(SENT).view(np.uint32)).any(), "a destination element was not written"
        return out


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def device_plan(c, stream=None, **over):
    """-> (rc, ws tensor, counts)"""
    lib, P = _lib(), c.P
    nbytes = ctypes.c_int64(0)
    assert lib.gsr_densify_plan_bytes(P, ctypes.byref(nbytes)) == 0, _err()
    ws = torch.empty((nbytes.value + 15) // 16 * 2, dtype=torch.int64, device="cuda")
    ins = [_dev(c.accum), _dev(c.denom), _dev(c.tensors["scaling"]), _dev(c.tensors["opacity"]), _dev(c.radii)]
    kw = dict(max_grad=DC.MAX_GRAD, min_opacity=DC.MIN_OPACITY, extent=DC.EXTENT, percent_dense=DC.PERCENT_DENSE,
              max_screen=c.max_screen or 0.0, N=c.N, flags=c.flags(), ws_bytes=ws.numel() * 8)
    kw.update(over)
    counts = (ctypes.c_int64 * 3)(-1, -1, -1)
    rc = lib.gsr_densify_plan(*[t.data_ptr() if P else None for t in ins], P, kw["max_grad"], kw["min_opacity"], kw["extent"],
                              kw["percent_dense"], kw["max_screen"], kw["N"], kw["flags"], ws.data_ptr(), kw["ws_bytes"], counts,
                              stream or _stream())
    return rc, ws, [int(v) for v in counts]


class DeviceRun:
    """one plan + apply of a case through the C ABI on guarded buffers"""

    def __init__(self, name, keyed=False, shift=None, stream=None, sync=True):
        c = self.c = DC.case(name)
        rc, self.ws, self.counts = device_plan(c, stream)
        assert rc == 0, _err()
        Pn = self.rows = self.counts[0] + self.counts[1] + c.N * self.counts[2]
        names = self.names = DC.live_names(c)
        sh = shift or {}
        self.src = {k: Guarded(c.tensors[k].shape, c.tensors[k], sh.get(k, 0)) for k in names}
        self.msrc = {k: tuple(Guarded(a.shape, a, sh.get(k + ".m", sh.get(k, 0))) for a in c.moments[k]) for k in names if k in c.moments}
        self.dst = {k: Guarded((Pn, c.tensors[k].shape[1]), None, sh.get(k + ".dst", 0)) for k in names}
        self.mdst = {k: tuple(Guarded((Pn, c.tensors[k].shape[1])) for _ in range(2)) for k in self.msrc}
        self.rot = _dev(c.tensors["rotation"])
        self.normals = None if keyed else _dev(c.normals)
        self.mask_in = None if c.mask is None else _dev(c.mask)
        self.mask_out = torch.full((Pn + 2 * PAD,), 77, dtype=torch.uint8, device="cuda")
        self.origin = torch.full((Pn + 2 * PAD,), -5, dtype=torch.int32, device="cuda")
        self.kind = torch.full((Pn + 2 * PAD,), -5, dtype=torch.int32, device="cuda")
        self.rc = self.call(stream)
        if sync:
            torch.cuda.synchronize()

    def call(self, stream=None, **over):
        c, names, n = self.c, self.names, len(self.names)
        arr = lambda vals: (ctypes.c_void_p * max(n, 1))(*vals)   # noqa: E731
        has = bool(self.msrc)
        mom = lambda d, i: arr([d[k][i].ptr if k in d else None for k in names]) if has else None   # noqa: E731
        kw = dict(ws=self.ws.data_ptr(), ws_bytes=self.ws.numel() * 8, P=c.P, counts=self.counts, n=n,
                  src=arr([self.src[k].ptr for k in names]), dst=arr([self.dst[k].ptr for k in names]),
                  cols=[c.tensors[k].shape[1] for k in names], roles=[DC.ROLES.get(k, DC.COPY) for k in names], N=c.N,
                  rot=self.rot.data_ptr() if c.P else None)
        kw.update(over)
        return _lib().gsr_densify_apply(kw["ws"], kw["ws_bytes"], kw["P"], (ctypes.c_int64 * 3)(*kw["counts"]), kw["n"], kw["src"], kw["dst"],
                                        mom(self.msrc, 0), mom(self.msrc, 1), mom(self.mdst, 0), mom(self.mdst, 1),
                                        (ctypes.c_int32 * max(len(kw["cols"]), 1))(*kw["cols"]),
                                        (ctypes.c_int32 * max(len(kw["roles"]), 1))(*kw["roles"]), kw["rot"], kw["N"], c.seed,
                                        None if self.normals is None else self.normals.data_ptr(),
                                        None if self.mask_in is None else self.mask_in.data_ptr(), self.mask_out.data_ptr() + PAD,
                                        self.origin.data_ptr() + 4 * PAD, self.kind.data_ptr() + 4 * PAD, stream or _stream())

    def result(self):
        """the dict of densify_cases.host_run; asserts the sentinels, full coverage and that no source was written"""
        c, Pn = self.c, self.rows
        assert self.rc == 0, _err()
        out = {k: self.dst[k].get() for k in self.names}
        mo = {k: (self.mdst[k][0].get(), self.mdst[k][1].get()) for k in self.mdst}
        for k in self.names:
            assert DC.same(self.src[k].get(), c.tensors[k]), f"{c.name}: the source {k} was written"
            if k in self.msrc:
                assert DC.same(self.msrc[k][0].get(), c.moments[k][0]) and DC.same(self.msrc[k][1].get(), c.moments[k][1])
        for k in DC.NAMES:
            if k not in out:
                out[k] = np.zeros((Pn, 0), np.float32)
                if k in c.moments:
                    mo[k] = (out[k], out[k])
        ints = []
        for t, fill in ((self.mask_out, 77), (self.origin, -5), (self.kind, -5)):
            h = t.cpu().numpy()
            assert (h[:PAD] == fill).all() and (h[PAD + Pn:] == fill).all(), "entries around mask / origin / kind were written"
            ints.append(h[PAD:PAD + Pn].copy())
        assert (ints[0] <= 1).all() and (ints[1] >= 0).all() and (ints[2] >= 0).all(), "a row of mask / origin / kind was not written"
        return dict(tensors=out, moments=mo, mask=ints[0], origin=ints[1], kind=ints[2], rows=Pn, counts=self.counts)


def assert_host_bits(c, got, host, keyed=False):
    assert got["counts"] == host["counts"], (c.name, got["counts"], host["counts"])
    assert np.array_equal(got["origin"], host["origin"]) and np.array_equal(got["kind"], host["kind"]), c.name
    assert np.array_equal(got["mask"], host["mask"]), (c.name, "row mask")
    ch = host["kind"] >= 2
    for k in DC.NAMES:
        rows = ~ch if k == "xyz" else np.ones(len(ch), bool)           # child scales included: raw - c is one operation
        assert DC.same(got["tensors"][k][rows], host["tensors"][k][rows]), (c.name, k)
        assert (k in got["moments"]) == (k in host["moments"])
        if k in host["moments"]:
            assert DC.same(got["moments"][k][0], host["moments"][k][0]) and DC.same(got["moments"][k][1], host["moments"][k][1]), (c.name, k, "moments")
    normals = DC.host_normals(c.seed, c.P, c.N) if keyed else c.normals
    e = DC.position_bound(c, host["origin"], host["kind"], normals, keyed=keyed, device=True)      # e_dev: only expf (and logf) differ
    gp, hp = got["tensors"]["xyz"][ch].astype(np.float64), host["tensors"]["xyz"][ch].astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(e) & np.isfinite(hp)
        worst = float(np.max(np.abs(gp - hp)[ok] / e[ok])) if ok.any() else 0.0
    assert worst <= 1.0, (c.name, "child positions against the host build: error / bound", worst)
    assert DC.same(got["tensors"]["xyz"][ch][~ok], host["tensors"]["xyz"][ch][~ok]), (c.name, "non-finite child positions: class and bits")
    return worst


# ---- every case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.ALL)
def test_case_matches_the_host_build_and_the_oracle(name):
    c = DC.case(name)
    run = DeviceRun(name)
    got = run.result()
    w_host = assert_host_bits(c, got, DC.host_run(name))
    w_ref = DC.check_against_oracle("device", c, got, DC.oracle(name))
    again = DeviceRun(name).result()                                   # run to run: the same bits
    assert all(DC.same(again["tensors"][k], got["tensors"][k]) for k in DC.NAMES), (name, "a second run differs")
    assert np.array_equal(again["origin"], got["origin"]) and np.array_equal(again["kind"], got["kind"])
    print(f"densify device {name}: rows {c.P} -> {got['rows']}, position error / bound {w_host:.3f} (host) {w_ref:.3f} (oracle)")


def test_children_of_rows_with_an_infinite_or_overflowing_scale():
    """nonfinite-open: the children exist, their scale is +inf or the finite raw - c, their positions are the host build's bits"""
    name, R = "nonfinite-open", DC.NONFINITE_ROWS
    c, got, host = DC.case(name), DeviceRun(name).result(), DC.host_run(name)
    for row, scale0 in (("inf_scale_hot", None), ("overflow_scale", np.float32(100.0) - np.float32(np.log(0.8 * c.N)))):
        m = (got["origin"] == R[row]) & (got["kind"] >= 2)
        assert m.sum() == c.N, row
        sc, xyz = got["tensors"]["scaling"][m], got["tensors"]["xyz"][m]
        if scale0 is None:
            assert np.isposinf(sc[:, 1]).all() and np.isfinite(sc[:, [0, 2]]).all()
        else:
            assert (sc[:, 0] == scale0).all() and np.isfinite(sc).all()
        assert not np.isfinite(xyz).any() and DC.same(xyz, host["tensors"]["xyz"][m]) and DC.same(sc, host["tensors"]["scaling"][m])


@pytest.mark.parametrize("name", ["size-P65-N2", "size-P2049-N3", "size-P6151-N2", "mix-all-split", "N8", "state-none"])
def test_keyed_normals_match_the_host_build(name):
    c = DC.case(name)
    got = DeviceRun(name, keyed=True).result()
    host = DC.host_run(name, True)
    w = assert_host_bits(c, got, host, keyed=True)
    assert DC.same(DeviceRun(name, keyed=True).result()["tensors"]["xyz"], got["tensors"]["xyz"])
    ch = host["kind"] >= 2
    assert ch.sum() >= 2 and not DC.same(got["tensors"]["xyz"][ch], DC.host_run(name)["tensors"]["xyz"][ch])     # not the given normals
    print(f"densify device keyed {name}: position error / bound {w:.3f}")


@pytest.mark.parametrize("floats", [1, 2, 3])
@pytest.mark.parametrize("name", ["mask", "size-P2049-N2"])
def test_every_tensor_off_the_16_byte_boundary(name, floats):
    """every source, moment and destination 4, 8 and 12 bytes past a 16-byte boundary (the 4-byte path); then the moments alone
    (a group whose parameter is aligned and whose state is not)"""
    c = DC.case(name)
    names = DC.live_names(c)
    host = DC.host_run(name)
    every = {k: floats for k in names}
    every.update({k + ".dst": floats for k in names})
    assert_host_bits(c, DeviceRun(name, shift=every).result(), host)
    assert_host_bits(c, DeviceRun(name, shift={k + ".m": floats for k in names}).result(), host)
    assert_host_bits(c, DeviceRun(name, shift={"f_rest": floats, "xyz": floats}).result(), host)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    c = DC.case("mask")
    for kw, word in ((dict(N=0), "N="), (dict(N=9), "N="), (dict(max_grad=float("nan")), "max_grad"), (dict(max_grad=1e39), "max_grad"),
                     (dict(extent=0.0), "extent"), (dict(extent=-1.0), "extent"), (dict(extent=float("inf")), "extent"),
                     (dict(percent_dense=0.0), "extent"), (dict(min_opacity=0.0), "min_opacity"), (dict(min_opacity=1.0), "min_opacity"),
                     (dict(min_opacity=float("nan")), "min_opacity"), (dict(flags=4), "flags"), (dict(ws_bytes=64), "workspace")):
        rc, _, counts = device_plan(c, **kw)
        assert rc == GSR_ERR_INVALID and word in _err(), (kw, _err())
    nbytes = ctypes.c_int64(0)
    assert _lib().gsr_densify_plan_bytes((1 << 28) + 1, ctypes.byref(nbytes)) == GSR_ERR_INVALID and "2^28" in _err()
    run = DeviceRun("mask")
    want = run.result()
    n = len(run.names)
    one = lambda v: (ctypes.c_void_p * n)(*v)   # noqa: E731
    src_ptrs = [run.src[k].ptr for k in run.names]
    for kw, word in ((dict(N=0), "N="), (dict(N=9), "N="), (dict(n=9), "tensors"), (dict(cols=[49] + [1] * (n - 1)), "cols"),
                     (dict(cols=[0] + [1] * (n - 1)), "cols"), (dict(dst=one(src_ptrs)), "overlaps"),
                     (dict(dst=one([run.dst[run.names[0]].ptr] + src_ptrs[1:])), "overlaps"),
                     (dict(dst=one([run.normals.data_ptr()] + [run.dst[k].ptr for k in run.names[1:]])), "the normals"),
                     (dict(dst=one([run.rot.data_ptr()] + [run.dst[k].ptr for k in run.names[1:]])), "the rotation"),
                     (dict(dst=one([run.ws.data_ptr()] + [run.dst[k].ptr for k in run.names[1:]])), "the workspace"),
                     (dict(dst=one([run.origin.data_ptr() + 4 * PAD] + [run.dst[k].ptr for k in run.names[1:]])), "two outputs"),
                     (dict(P=(1 << 28) + 1), "2^28"),
                     (dict(counts=[run.c.P, run.c.P, run.c.P + 1]), "counts"), (dict(ws_bytes=64), "workspace"),
                     (dict(roles=[7] * n), "role"), (dict(rot=None), "rotation")):
        assert run.call(**kw) == GSR_ERR_INVALID and word in _err(), (kw, _err())
    # P' above 2^28 from counts that each fit
    big = (1 << 28) - 1
    assert run.call(P=big + 1, counts=[big, big, 0]) == GSR_ERR_INVALID and "P'" in _err()
    torch.cuda.synchronize()
    after = run.result()                                               # nothing ran after the one good call
    assert all(DC.same(after["tensors"][k], want["tensors"][k]) for k in DC.NAMES)


def test_binding_refuses_what_the_kernel_does_not_take():
    from diff_gaussian_rasterization import densify_ops as DO
    assert DO.available()
    P = 10
    z = torch.zeros(P, device="cuda")
    with pytest.raises(RuntimeError, match="HIP device"):
        DO.plan(z.cpu(), z.cpu(), torch.zeros(P, 3), z.cpu(), max_grad=1.0, min_opacity=0.5, extent=1.0, percent_dense=0.01)
    with pytest.raises(ValueError, match="contiguous float32"):
        DO.plan(z.double(), z, torch.zeros(P, 3, device="cuda"), z, max_grad=1.0, min_opacity=0.5, extent=1.0, percent_dense=0.01)
    with pytest.raises(ValueError, match="min_opacity"):
        DO.plan(z, z, torch.zeros(P, 3, device="cuda"), z, max_grad=1.0, min_opacity=0.0, extent=1.0, percent_dense=0.01)
    pl = DO.plan(z, z + 1, torch.zeros(P, 3, device="cuda"), z, max_grad=1.0, min_opacity=0.5, extent=1.0, percent_dense=0.01)
    assert (pl.n_keep, pl.n_clone, pl.n_split) == (P, 0, 0)
    with pytest.raises(ValueError, match="columns"):
        DO.apply(pl, [(torch.zeros(P, 49, device="cuda"), None, None, DO.COPY)], torch.zeros(P, 4, device="cuda"))


# ---- streams ----------------------------------------------------------------------------------------------------------------------
def test_two_streams_give_the_sequential_bits():
    names = ("size-P4097-N2", "size-P2049-N3")
    want = [DeviceRun(n).result() for n in names]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    runs = []
    for n, s in zip(names, streams):
        with torch.cuda.stream(s):
            runs.append(DeviceRun(n, stream=ctypes.c_void_p(s.cuda_stream), sync=False))
    torch.cuda.synchronize()
    for r, w in zip(runs, want):
        got = r.result()
        assert got["counts"] == w["counts"] and np.array_equal(got["origin"], w["origin"])
        assert all(DC.same(got["tensors"][k], w["tensors"][k]) for k in DC.NAMES)
        assert all(DC.same(got["moments"][k][i], w["moments"][k][i]) for k in w["moments"] for i in (0, 1))


# ---- the statistics -----------------------------------------------------------------------------------------------------------------
def _stats_inputs(P, B, seed):
    r = np.random.default_rng(seed)
    grad = (r.normal(0, 1e-3, (B, P, 3)) * np.exp(r.normal(0, 2, (B, P, 1)))).astype(np.float32)
    radii = (r.integers(0, 60, (B, P)) * (r.random((B, P)) < 0.7)).astype(np.int32)
    accum = r.uniform(0, 1e-2, P).astype(np.float32)
    denom = r.integers(0, 9, P).astype(np.float32)
    maxr = r.integers(0, 40, P).astype(np.float32)
    return grad, radii, accum, denom, maxr


def _host_stats(grad, radii, flt, accum, denom, maxr):
    a, d, m = accum.copy(), denom.copy(), None if maxr is None else maxr.copy()
    B, P = grad.shape[0], grad.shape[1]
    rc = DC.host_lib().dh_stats(grad.ctypes.data, None if radii is None else radii.ctypes.data, None if flt is None else flt.ctypes.data, B, P,
                                a.ctypes.data, d.ctypes.data, None if m is None else m.ctypes.data)
    assert rc == 0
    return a, d, m


@pytest.mark.parametrize("P", [1, 63, 257, 2049])
def test_statistics_are_the_host_builds_bits_and_a_batch_equals_single_calls(P):
    from diff_gaussian_rasterization import densify_ops as DO
    B = 3
    grad, radii, accum, denom, maxr = _stats_inputs(P, B, P)
    ha, hd, hm = _host_stats(grad, radii, None, accum, denom, maxr)
    assert (hd != denom).sum() >= P // 2 and (hd == denom).sum() >= (1 if P > 60 else 0)      # most rows seen, some never
    dev = lambda a: torch.from_numpy(a.copy()).cuda()   # noqa: E731
    a, d, m = dev(accum)[:, None], dev(denom)[:, None], dev(maxr)
    DO.stats_(dev(grad), a, d, radii=dev(radii), max_radii=m)
    torch.cuda.synchronize()
    assert DC.same(a.cpu().numpy(), ha) and DC.same(d.cpu().numpy(), hd) and DC.same(m.cpu().numpy(), hm)
    a1, d1, m1 = dev(accum), dev(denom), dev(maxr)
    for b in range(B):
        DO.stats_(dev(grad[b]), a1, d1, radii=dev(radii[b]), max_radii=m1)
    assert torch.equal(a1, a.reshape(-1)) and torch.equal(d1, d.reshape(-1)) and torch.equal(m1, m)
    # an explicit filter, without radii: the reference's add_densification_stats
    flt = (np.random.default_rng(P + 1).random((B, P)) < 0.5)
    ha, hd, _ = _host_stats(grad, None, flt.astype(np.uint8), accum, denom, None)
    a2, d2 = dev(accum), dev(denom)
    DO.stats_(dev(grad), a2, d2, update_filter=dev(flt))
    assert DC.same(a2.cpu().numpy(), ha) and DC.same(d2.cpu().numpy(), hd)
    # and torch.norm in float64: three roundings (two products' sum, the root) on |g|, one per addition
    want = accum.astype(np.float64) + sum(np.where(flt[b], np.linalg.norm(grad[b, :, :2].astype(np.float64), axis=1), 0.0) for b in range(B))
    assert (np.abs(ha - want) <= 4 * B * DC.U * np.abs(want) + 1e-45).all()


# ---- the model's route --------------------------------------------------------------------------------------------------------------
def _model_pair(P=500, frozen=False, mask=False):
    from gsplat_attack.optim import OptimizationParams
    from gsplat_attack.scenes import make_scene
    pair = []
    for dev in ("cuda", "cpu"):
        model, cams, _ = make_scene("hydrant-1k", device=dev, P=P, n_views=1, width=64, height=64)
        with torch.no_grad():
            model._opacity[::11] = -7.0                                # rows a densify prunes: sigmoid(-7) < 0.005
        if frozen:
            sel = torch.arange(P) % 3 != 0
            model.finetune_setup(OptimizationParams(), sel.to(dev))
        else:
            model.training_setup(OptimizationParams())
        pair.append(model)
    return pair


def _fake_step(models, seed):
    """the same gradients on both models, one optimiser step each"""
    g = torch.Generator().manual_seed(seed)
    for name, p in models[1].named_parameters().items():
        if not p.requires_grad:
            continue
        grad = torch.randn(p.shape, generator=g) * 1e-2
        for m in models:
            m.named_parameters()[name].grad = grad.to(m._xyz.device)
    for m in models:
        m.optimizer.step()
        m.optimizer.zero_grad()


def _sync_host(models):
    """the host copy takes the device's bits (the tensor-op Adam step may leave an element of x an ulp away: tests/test_adam_host_cpu.py);
    the moments agree bit for bit already"""
    with torch.no_grad():
        for a, b in zip(models[0].parameters(), models[1].parameters()):
            assert torch.allclose(a.cpu(), b, rtol=1e-5, atol=1e-7)
            b.copy_(a.cpu())
    for name, st in models[0].optimizer.state.items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k].cpu(), models[1].optimizer.state[name][k]) and st[k].any()


@pytest.mark.parametrize("frozen", [False, True])
def test_model_route_against_the_host_route(frozen):
    """two Adam steps, densify_and_prune, two more steps: the device model against a CPU copy through the tensor-op branch.
    The moments of kept rows continue, those of new rows start at zero."""
    models = _model_pair(frozen=frozen)
    P = 500
    _fake_step(models, 1)
    _fake_step(models, 2)
    _sync_host(models)
    g = torch.Generator().manual_seed(3)
    vs = torch.randn(P, 3, generator=g) * 4e-4
    seen = torch.rand(P, generator=g) < 0.8
    radii = (torch.randint(1, 50, (P,), generator=g) * seen).to(torch.int32)
    for m in models:
        d = m._xyz.device
        m.add_densification_stats(vs.to(d), seen.to(d), radii=radii.to(d))
    assert torch.equal(models[0].xyz_gradient_accum.cpu(), models[1].xyz_gradient_accum)
    assert torch.equal(models[0].max_radii2D.cpu(), models[1].max_radii2D)
    m_before = models[0].optimizer.state["xyz"]["exp_avg"].clone()
    before = types.SimpleNamespace(tensors={k: getattr(models[1], a).detach().numpy().reshape(P, -1).copy()
                                            for k, a in (("xyz", "_xyz"), ("scaling", "_scaling"), ("rotation", "_rotation"))})
    old_params = list(models[0].parameters())
    out = [m.densify_and_prune(0.0002, 0.005, 3.0, 20) for m in models]
    (og, kg), (oc, kc) = out
    assert torch.equal(og.cpu(), oc) and torch.equal(kg.cpu(), kc)
    n_new = int((kc > 0).sum())
    assert int((kc == 1).sum()) >= 20 and int((kc >= 2).sum()) >= 20 and int((kc == 0).sum()) < P      # clones, children, and rows gone
    assert not np.isin(np.arange(0, P, 11), oc.numpy()).any()                                            # the pruned rows yield nothing
    Pn = kc.numel()
    for m in models:
        assert m._xyz.shape[0] == Pn and m.xyz_gradient_accum.shape == (Pn, 1) and not m.denom.any() and m.max_radii2D.shape == (Pn,)
        assert m.densify_count == 1
    assert all(p is not q for p in models[0].parameters() for q in old_params)
    child = kc >= 2
    for (name, a), b in zip(models[0].named_parameters().items(), models[1].parameters()):
        a, b = a.detach().cpu(), b.detach()
        assert a.shape == b.shape and a.requires_grad == b.requires_grad
        if name == "xyz":
            assert torch.equal(a[~child], b[~child])
            # the tensor-op branch is another implementation (torch's vectorised root and exp, numpy's log), not the header's
            # build: both lie within e_pos of the exact value, per row, plus the keyed normals' term
            e = DC.position_bound(before, oc.numpy(), kc.numpy(), DC.host_normals(0, P, 2), keyed=True, factor=2.0)
            assert np.isfinite(e).all() and (np.abs(a[child].double().numpy() - b[child].double().numpy()) <= e).all()
        else:
            assert torch.equal(a, b), name
    for name, st in models[1].optimizer.state.items():
        sg = models[0].optimizer.state[name]
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sg[k].cpu(), st[k]), (name, k)
            assert not st[k][kc > 0].any() and (n_new == 0 or st[k][kc == 0].any())
    keep = (kc == 0)
    assert torch.equal(models[0].optimizer.state["xyz"]["exp_avg"][keep.cuda()], m_before[og[keep.cuda()].long()])
    if frozen:
        assert "obj_dc" not in models[0].optimizer.state and not models[0]._objects_dc.requires_grad
        lg, lc = models[0].optimizer.row_mask.cpu(), models[1].optimizer.row_mask
        assert torch.equal(lg, lc) and lc[kc > 0].all() and torch.equal(lc[keep], (torch.arange(P) % 3 != 0)[oc[keep].long()].to(torch.uint8))
    _fake_step(models, 4)
    _fake_step(models, 5)
    for (name, a), b in zip(models[0].named_parameters().items(), models[1].parameters()):
        if name != "xyz":
            assert torch.allclose(a.detach().cpu(), b.detach(), rtol=1e-5, atol=1e-6), name
    assert models[0].optimizer.step_count == 4


def test_prune_points_is_the_fused_prune():
    models = _model_pair(P=300)
    _fake_step(models, 1)
    _sync_host(models)
    mask = torch.rand(300, generator=torch.Generator().manual_seed(9)) < 0.4
    for m in models:
        m.xyz_gradient_accum += 1.5
        m.prune_points(mask.to(m._xyz.device))
    keep = ~mask
    for a, b in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(a.detach().cpu(), b.detach()) and a.shape[0] == int(keep.sum())
    for name, st in models[1].optimizer.state.items():
        assert torch.equal(models[0].optimizer.state[name]["exp_avg_sq"].cpu(), st["exp_avg_sq"])
    assert torch.equal(models[0].xyz_gradient_accum.cpu(), models[1].xyz_gradient_accum) and bool((models[1].xyz_gradient_accum == 1.5).all())


def test_render_after_a_densify_sees_the_new_rows():
    import diff_gaussian_rasterization as D
    from gsplat_attack.optim import OptimizationParams
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device="cuda", P=400, n_views=1, width=64, height=64)
    model.training_setup(OptimizationParams())
    cache = D.RenderCache()
    pipe = PipelineParams(skip_objects=True, render_cache=cache)
    bg = torch.zeros(3, device="cuda")
    out = render(cams[0], model, pipe, bg)
    out["render"].sum().backward()
    assert out["radii"].shape[0] == 400
    with torch.no_grad():
        model.add_densification_stats(out["viewspace_points"], None, radii=out["radii"])
        model.xyz_gradient_accum += 1.0                                # every seen row hot
        origin, kind = model.densify_and_prune(0.0002, 0.005, 1.0, None)
    Pn = int(kind.numel())
    assert Pn > 400 and model._xyz.shape[0] == Pn
    again = render(cams[0], model, pipe, bg)
    assert again["radii"].shape[0] == Pn and again["viewspace_points"].shape[0] == Pn                 # no stale render cache
    assert int((again["radii"] > 0).sum()) > 0
    again["render"].sum().backward()
    assert model._xyz.grad.shape[0] == Pn


def test_refit_with_a_densify_schedule_grows_prunes_and_repeats_bit_for_bit():
    from gsplat_attack.densify import DensifyParams
    from gsplat_attack.optim import OptimizationParams, refit
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene

    def fit():
        model, cams, _ = make_scene("hydrant-1k", device="cuda", P=600, n_views=4, width=64, height=64)
        bg = torch.zeros(3, device="cuda")
        with torch.no_grad():
            targets = [render(c, model, PipelineParams(skip_objects=True), bg)["render"].detach() for c in cams]
            model._xyz.add_(0.05 * torch.randn(model._xyz.shape, generator=torch.Generator().manual_seed(1)).cuda())
            model._opacity[::7] = -7.0                                 # some rows a densify prunes
        model.training_setup(OptimizationParams())
        sizes = []
        orig = model.densify_and_prune

        def spy(*a, **k):
            before = int(model._xyz.shape[0])
            o, kd = orig(*a, **k)
            sizes.append((before, int((kd == 0).sum()), int((kd > 0).sum())))
            return o, kd
        model.densify_and_prune = spy
        dp = DensifyParams(densify_from_iter=5, densify_until_iter=30, densification_interval=8, opacity_reset_interval=20,
                           densify_grad_threshold=1e-6, sh_degree_interval=10, extent=2.0)
        losses = refit(model, cams, targets, iters=36, densify=dp)
        return model, sizes, losses

    m1, sizes, l1 = fit()
    assert len(sizes) == 3                                            # iterations 8, 16, 24
    assert any(kept < before for before, kept, new in sizes) and any(new > 0 for _, _, new in sizes)    # pruned, and grew
    assert m1._xyz.shape[0] != 600 and m1.densify_count == 3
    m2, sizes2, l2 = fit()
    assert sizes2 == sizes and torch.equal(l1, l2)
    for a, b in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(a, b)

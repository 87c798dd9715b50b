"""Every batched-backward mode against every output buffer it writes.

One batch forward per case (through the C ABI with ctypes, so that the test owns every output buffer), then each backward
entry point that shares backward_impl: gsr_backward_raw_batch_into (fresh / accumulating), gsr_backward_raw_chunked on a
batch context (nchunks 2, 3, 5, more than ceil(P / 64); accumulating; on an object context with dL/dobjects),
gsr_backward_raw_batch_views, gsr_backward_raw_batch_obj_into (with and without dL/dobjects) and _obj_views -- each with
geometry and colour-only (every geometry pointer and dmeans2D null).

Every buffer is NaN before an overwriting call and a known random start before an accumulating one: a float that should
have been written and was not shows, and so does a float written where none belongs (the colour-only calls must leave the
geometry slices as they were).

No expected value comes from the mode under test.  The reference builder (_loop) takes parameters, settings and dL/dC --
never a batch context -- and runs gsr_forward_raw + gsr_backward_raw / _into per camera:
  dmeans2D[v], per-view gradients, per-view object gradients      bit-equal to view v's single-view backward
  dobjects_dc of the summing modes                                bit-equal to ((s_0 + s_1) + s_2) + ... in float32
  summed 59-float gradients                                       tests/test_gpu_batch.py's yardstick (_yard below)
  a chunked call                                                  also bit-equal, in every buffer, to the unchunked call
One chunked geometry case and one chunked object case are held against oracle-R in float64 as well.

The scene (_scene) is laid out so that chunk boundaries and views matter: parallel cameras that each see a cluster of their
own plus a far cluster they all see, a view that sees nothing, and index ranges no view sees; Gaussians change group every
32 indices, so every range of 64 mixes the views.  The test asserts those properties from the forward's radii."""
import ctypes
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

W, H = 333, 190                                    # no multiple of a tile: partial tiles on two edges
CUTS = (0, 3, 6, 51, 52, 55, 59)                   # xyz | f_dc | f_rest | opacity | scaling | rotation (GradBucket's layout)
GNAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
COLOUR = (1, 2)                                    # the slices a colour-only backward writes
BG = (0.15, 0.3, 0.45)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------------
def _blind_view(B):
    return 1 if B >= 3 else None


def _scene(P, B, seed):
    """-> (dict of raw parameter tensors on the CPU, cameras).  Groups by index, 32 at a time, in the repeating pattern
    common | private 0 | ... | private n-1 | hidden x 3: three hidden blocks in a row always hold an aligned range of 64."""
    from gsplat_attack.cameras import look_at_camera
    g = torch.Generator().manual_seed(seed)
    blind = _blind_view(B)
    seeing = [v for v in range(B) if v != blind]
    n = len(seeing)
    pattern = torch.tensor([0] + list(range(1, n + 1)) + [n + 1] * 3)
    grp = pattern[(torch.arange(P) // 32) % pattern.numel()]
    step = 5.0
    mid = 0.5 * step * (n - 1)
    centre = torch.zeros(n + 2, 3)
    half = torch.zeros(n + 2)
    centre[0] = torch.tensor([mid, 200.0, 0.0]); half[0] = 5.0                    # far away: every seeing camera sees it
    for k in range(n):
        centre[1 + k] = torch.tensor([step * k, 8.0, 0.0]); half[1 + k] = 0.5     # in front of camera k only
    centre[n + 1] = torch.tensor([mid, -50.0, 0.0]); half[n + 1] = 2.0            # behind every camera
    u = lambda *s: torch.rand(*s, generator=g)
    xyz = centre[grp] + half[grp, None] * (2.0 * u(P, 3) - 1.0)
    base = torch.where(grp == 0, torch.tensor(0.3), torch.tensor(0.02))[:, None]
    scaling = torch.log(base * (1.0 + 5.0 * u(P, 3)))
    params = dict(xyz=xyz, dc=0.5 + 0.5 * torch.randn(P, 1, 3, generator=g), rest=0.1 * torch.randn(P, 15, 3, generator=g),
                  obj=torch.randn(P, 16, generator=g), op=-2.0 + 5.0 * u(P), sc=scaling, ro=torch.randn(P, 4, generator=g))
    cams = []
    for v in range(B):
        if v == blind:
            cams.append(look_at_camera((0.0, 0.0, 50.0), (0.0, 0.0, 60.0), up=(0.0, 1.0, 0.0), fovx=2.0 * math.atan(0.3),
                                       width=W, height=H, uid=v))
        else:
            x = step * seeing.index(v)
            cams.append(look_at_camera((x, 0.0, 0.0), (x, 1.0, 0.0), up=(0.0, 0.0, 1.0), fovx=2.0 * math.atan(0.3),
                                       width=W, height=H, uid=v))
    return params, cams


class _Case:
    """Parameters, settings and dL/dC, dL/dobjects of one (P, B) on the device, its two batch contexts and the references
    already computed (the matrix asks for each of them many times)."""

    def __init__(self, P, B, dev, params=None, cams=None, w=W, h=H, flags=0):
        import diff_gaussian_rasterization as D
        from util import settings_for
        self.P, self.B, self.dev, self.w, self.h = P, B, dev, w, h
        if params is None:
            params, cams = _scene(P, B, seed=1000 * B + P)
        self.par = {k: t.detach().float().contiguous().to(dev) for k, t in params.items()}
        self.bg = torch.tensor(BG, device=dev)
        self.cams = list(cams)                      # (CPU tensors: settings_for moves them)
        self.lib = D._load()
        with D.extra_flags(flags):
            self.packs = [D._SettingsPack(settings_for(c, self.bg, 3, 1.0, cls=D.GaussianRasterizationSettings, device=dev), dev)
                          for c in self.cams]
        g = torch.Generator().manual_seed(7 * P + B)
        self.gc = torch.randn(B, 3, h, w, generator=g).to(dev)
        self.go = torch.randn(B, 16, h, w, generator=g).to(dev)
        self.start = (3.0 * torch.randn(59 * P, generator=g)).to(dev)
        self.ctx, self.ref = {}, {}

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def batch(self, with_obj):
        """The batch forward (once per kind of context) -> (holder, radii [B,P], image, object map or None)."""
        import diff_gaussian_rasterization as D
        if with_obj in self.ctx:
            return self.ctx[with_obj]
        p, B, P, dev, lib = self.par, self.B, self.P, self.dev, self.lib
        carr = (D._CSettings * B)()
        for v, pk in enumerate(self.packs):
            carr[v] = pk.c
        color = torch.full((B, 3, self.h, self.w), float("nan"), device=dev)
        radii = torch.full((B, P), -1, dtype=torch.int32, device=dev)
        objects = torch.full((B, 16, self.h, self.w), float("nan"), device=dev) if with_obj else None
        handle, nren = ctypes.c_void_p(None), ctypes.c_int64(0)
        q = lambda t: ctypes.c_void_p(t.data_ptr())
        if with_obj:
            rc = lib.gsr_forward_raw_batch_obj(carr, B, P, q(p["xyz"]), q(p["dc"]), q(p["rest"]), q(p["obj"]), q(p["op"]),
                                               q(p["sc"]), q(p["ro"]), q(color), q(objects), q(radii), ctypes.byref(handle),
                                               ctypes.byref(nren), self.stream())
        else:
            rc = lib.gsr_forward_raw_batch(carr, B, P, q(p["xyz"]), q(p["dc"]), q(p["rest"]), q(p["op"]), q(p["sc"]),
                                           q(p["ro"]), q(color), q(radii), ctypes.byref(handle), ctypes.byref(nren),
                                           self.stream())
        assert rc == 0, D._err(lib)
        torch.cuda.synchronize()
        self.ctx[with_obj] = (D._CtxHolder(lib, handle), radii, color, objects, int(nren.value))
        return self.ctx[with_obj]


_CASES = {}

# The (192, 3) case: the ordinary scene with four Gaussians made so large that each has more partial rows in a seeing
# view than K8+K9 stages per round (ROW_CHUNK = 128), so that the whole wave sums them: a large one among small ones, one
# in a wave's last lane, one in the next wave's first lane, and a wave with a single large one.
WIDE_PB = (192, 3)
WIDE = (5, 63, 64, 130)
ROW_CHUNK = 128


def _wide_scene(P, B):
    params, cams = _scene(P, B, seed=1000 * B + P)
    seeing = [v for v in range(B) if v != _blind_view(B)]
    mid = 0.5 * 5.0 * (len(seeing) - 1)             # between the seeing cameras, in front of them all
    for k, i in enumerate(WIDE):
        params["xyz"][i] = torch.tensor([mid, 20.0 + k, 0.0])
        params["sc"][i] = math.log(10.0 + k)        # sigma = half the distance: the footprint covers the 21 x 12 tiles
        params["op"][i] = 0.0                       # alpha 0.5: what lies behind still gets a gradient
    return params, cams


def _check_wide(case):
    """The premise of the case, from the batch context's storage-order scan of tiles touched (export item 9)."""
    P, B = case.P, case.B
    holder = case.batch(False)[0]
    ppad = holder.info(5)
    offg = torch.zeros(B * ppad + 1, dtype=torch.int32, device=case.dev)
    assert case.lib.gsr_ctx_export(holder.handle, 9, ctypes.c_void_p(offg.data_ptr()), 4 * offg.numel(), case.stream()) == 0
    torch.cuda.synchronize()
    offg = offg.cpu().long() & 0xFFFFFFFF
    tiles = (offg[1:] - offg[:-1]).view(B, ppad)[:, :P]
    wide = torch.zeros(P, dtype=torch.bool)
    wide[list(WIDE)] = True
    for v in range(B):
        if v == _blind_view(B):
            assert not bool(tiles[v].any()), "the blind view sees something"
        else:
            assert bool((tiles[v][wide] > ROW_CHUNK).all()), (v, tiles[v][wide])
            assert bool((tiles[v][~wide] <= ROW_CHUNK).all()), (v, int(tiles[v][~wide].max()))


def _case(P, B):
    key = (P, B)
    if key not in _CASES:
        if len(_CASES) >= 2:                        # (the matrix is ordered by case: keep the last two only)
            _CASES.pop(next(iter(_CASES)))
        if key == WIDE_PB:
            _CASES[key] = _Case(P, B, _dev(), *_wide_scene(P, B))
            _check_wide(_CASES[key])
        else:
            _CASES[key] = _Case(P, B, _dev())
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------------
class _Out:
    """n buckets of 59 P floats (one, or one per view), dmeans2D [B,P,3] and the object gradient [n,P,16]; all NaN, or the
    buckets at `start`."""

    def __init__(self, P, B, n, dev, start=None):
        self.P, self.n = P, n
        self.flat = torch.full((n, 59 * P), float("nan"), device=dev)
        if start is not None:
            self.flat.copy_(start.view(1, -1).expand(n, -1))
        self.dm2 = torch.full((B, P, 3), float("nan"), device=dev)
        self.dobj = torch.full((n, P, 16), float("nan"), device=dev)

    def sl(self, i, v=0):
        return self.flat[v, CUTS[i] * self.P:CUTS[i + 1] * self.P]

    def ptrs(self, geom, obj):
        """(dxyz, dmeans2D, dfeatures_dc, dfeatures_rest, dobjects_dc, dopacity, dscaling, drotation) as the C ABI orders
        them; colour-only: the geometry pointers and dmeans2D null."""
        q = lambda t: ctypes.c_void_p(t.data_ptr())
        n_ = ctypes.c_void_p(None)
        return (q(self.sl(0)) if geom else n_, q(self.dm2) if geom else n_, q(self.sl(1)), q(self.sl(2)),
                q(self.dobj) if obj else n_, q(self.sl(3)) if geom else n_, q(self.sl(4)) if geom else n_,
                q(self.sl(5)) if geom else n_)


def _same(a, b):
    """Bit-equal, NaN patterns included (a buffer nobody wrote must still be the NaN it was filled with)."""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: a loop of single-view calls.  Takes parameters, settings, dL/dC: never a batch context.
# ---------------------------------------------------------------------------------------------------------------------------
def _loop(lib, par, packs, w, h, gc, go, with_obj, geom, start=None):
    """Per camera gsr_forward_raw, then gsr_backward_raw into NaN buffers (the view's OWN gradients) and
    gsr_backward_raw_into on one shared bucket in view order (the first overwriting, or adding to `start`).
    -> dict(own [B,59P], dm2 [B,P,3], dobj [B,P,16] or None, seq [59P], exact [59P] float64, radii [B,P])."""
    import diff_gaussian_rasterization as D
    P, B, dev = int(par["xyz"].shape[0]), len(packs), par["xyz"].device
    q = lambda t: ctypes.c_void_p(None) if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    own = _Out(P, B, B, dev)
    seq = _Out(P, B, 1, dev, start)
    radii = torch.empty(B, P, dtype=torch.int32, device=dev)
    for v, pk in enumerate(packs):
        color = torch.empty(3, h, w, device=dev)
        objects = torch.empty(16, h, w, device=dev) if with_obj else None
        handle, nren = ctypes.c_void_p(None), ctypes.c_int64(0)
        rc = lib.gsr_forward_raw(ctypes.byref(pk.c), P, q(par["xyz"]), q(par["dc"]), q(par["rest"]),
                                 q(par["obj"] if with_obj else None), q(par["op"]), q(par["sc"]), q(par["ro"]), q(color),
                                 q(objects), q(radii[v]), ctypes.byref(handle), ctypes.byref(nren), stream)
        assert rc == 0, D._err(lib)
        holder = D._CtxHolder(lib, handle)
        gov = go[v] if (with_obj and go is not None) else None
        o = lambda i: q(own.sl(i, v)) if (geom or i in COLOUR) else q(None)
        rc = lib.gsr_backward_raw(holder.handle, q(gc[v]), q(gov), o(0), q(own.dm2[v]) if geom else q(None), o(1), o(2),
                                  q(own.dobj[v]) if with_obj else q(None), o(3), o(4), o(5), stream)
        assert rc == 0, D._err(lib)
        s = lambda i: q(seq.sl(i)) if (geom or i in COLOUR) else q(None)
        rc = lib.gsr_backward_raw_into(holder.handle, q(gc[v]), q(gov), s(0), q(None), s(1), s(2), q(None), s(3), s(4), s(5),
                                       1 if (v > 0 or start is not None) else 0, stream)
        assert rc == 0, D._err(lib)
        torch.cuda.synchronize()
        del holder
    exact = own.flat.double().sum(dim=0)
    if start is not None:
        exact = exact + start.double()
    return dict(own=own.flat, dm2=own.dm2, dobj=own.dobj if with_obj else None, seq=seq.flat[0], exact=exact, radii=radii)


def _ref(case, with_obj, with_go, geom, acc):
    key = (with_obj, with_go, geom, acc)
    if key not in case.ref:
        case.ref[key] = _loop(case.lib, case.par, case.packs, case.w, case.h, case.gc, case.go if with_go else None,
                              with_obj, geom, case.start if acc else None)
    return case.ref[key]


def _yard(got, ref, P, geom, what=""):
    """tests/test_gpu_batch.py:_check_equal's yardstick for the summed gradients: no further from the double sum of the
    per-view gradients than 3x the loop's own float32 accumulation, floors 1e-5 (1e-4: scale, rotation) of the tensor's
    largest gradient; bit-equality with the loop under GSR_BATCH_K9=0."""
    exact_bits = os.environ.get("GSR_BATCH_K9", "1") == "0"
    for i, name in enumerate(GNAMES):
        if not geom and i not in COLOUR:
            continue
        a, b = CUTS[i] * P, CUTS[i + 1] * P
        s2, s1, ex = got[a:b], ref["seq"][a:b], ref["exact"][a:b]
        assert bool(torch.isfinite(s2).all()), f"{what} {name}: {int((~torch.isfinite(s2)).sum())} floats not written"
        if exact_bits:
            assert torch.equal(s1, s2), f"{what} {name}: differs from the accumulated single-view gradients"
            continue
        scale_ = ex.abs().max().item()
        e_seq = (s1.double() - ex).abs().max().item()
        e_bat = (s2.double() - ex).abs().max().item()
        floor = 1e-4 if name in ("_scaling", "_rotation") else 1e-5
        print(f"{what} {name}: batch {e_bat:.3e}, loop {e_seq:.3e}, scale {scale_:.3e}")
        assert e_bat <= max(3.0 * e_seq, floor * scale_), f"{what} {name}: batch {e_bat:.3e}, loop {e_seq:.3e}, scale {scale_:.3e}"


def _untouched(out, before, geom, what):
    """Colour-only: the geometry slices of every bucket and dmeans2D hold what they held before the call."""
    if geom:
        return
    for v in range(out.n):
        for i in range(6):
            if i not in COLOUR:
                a, b = CUTS[i] * out.P, CUTS[i + 1] * out.P
                assert _same(out.flat[v, a:b], before[a:b]), f"{what}: a colour-only call wrote {GNAMES[i]} of bucket {v}"
    assert bool(torch.isnan(out.dm2).all()), f"{what}: a colour-only call wrote dmeans2D"


def _check_dm2(out, ref, geom, what):
    if not geom:
        return
    for v in range(ref["dm2"].shape[0]):
        bad = (out.dm2[v].view(torch.int32) != ref["dm2"][v].view(torch.int32)).any(dim=1)
        assert not bool(bad.any()), (f"{what}: dmeans2D of view {v} differs from the single-view backward in {int(bad.sum())} "
                                     f"rows, first {int(bad.nonzero()[0])}, of them NaN (never written) "
                                     f"{int(torch.isnan(out.dm2[v]).any(dim=1).sum())}")


def _view_sum(dobj):
    s = dobj[0].clone()
    for v in range(1, dobj.shape[0]):
        s = s + dobj[v]
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# the modes
# ---------------------------------------------------------------------------------------------------------------------------
def _call(case, mode, geom, with_go, acc, nchunks=0):
    """One backward of `mode` on the case's batch context into buffers this function fills first. -> (_Out, chunk ranges)."""
    import diff_gaussian_rasterization as D
    lib, P, B = case.lib, case.P, case.B
    with_obj = mode.startswith("obj")
    per_view = mode.endswith("views")
    holder = case.batch(with_obj)[0]
    out = _Out(P, B, B if per_view else 1, case.dev, case.start if acc else None)
    dx, dm2, ddc, drest, dobj, dop, dsc, dro = out.ptrs(geom, with_obj)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    gc, go = q(case.gc), (q(case.go) if with_go else ctypes.c_void_p(None))
    seen = []
    if nchunks:
        cb = D._CHUNK_FN(lambda _u, c, g0, g1: seen.append((int(c), int(g0), int(g1))))
        rc = lib.gsr_backward_raw_chunked(holder.handle, gc, go, dx, dm2, ddc, drest, dobj, dop, dsc, dro, 1 if acc else 0,
                                          nchunks, cb, None, case.stream())
    elif mode == "into":
        rc = lib.gsr_backward_raw_batch_into(holder.handle, gc, dx, dm2, ddc, drest, dop, dsc, dro, 1 if acc else 0,
                                             case.stream())
    elif mode == "views":
        rc = lib.gsr_backward_raw_batch_views(holder.handle, gc, dx, dm2, ddc, drest, dop, dsc, dro, 59 * P, case.stream())
    elif mode == "obj_into":
        rc = lib.gsr_backward_raw_batch_obj_into(holder.handle, gc, go, dx, dm2, ddc, drest, dobj, dop, dsc, dro,
                                                 1 if acc else 0, case.stream())
    elif mode == "obj_views":
        rc = lib.gsr_backward_raw_batch_obj_views(holder.handle, gc, go, dx, dm2, ddc, drest, dobj, dop, dsc, dro, 59 * P,
                                                  case.stream())
    else:
        raise AssertionError(mode)
    assert rc == 0, D._err(lib)
    torch.cuda.synchronize()
    return out, seen


def _check_mode(case, mode, geom, with_go=False, acc=False, nchunks=0):
    P, B = case.P, case.B
    with_obj = mode.startswith("obj")
    what = f"{mode}{' +dL/dobj' if with_go else ''}{' acc' if acc else ''}{f' chunks={nchunks}' if nchunks else ''} P={P} B={B}"
    ref = _ref(case, with_obj, with_go, geom, acc)
    out, seen = _call(case, mode, geom, with_go, acc, nchunks)
    before = case.start if acc else torch.full((59 * P,), float("nan"), device=case.dev)
    _untouched(out, before, geom, what)
    _check_dm2(out, ref, geom, what)
    if mode.endswith("views"):
        for v in range(B):
            for i in range(6):
                if geom or i in COLOUR:
                    a, b = CUTS[i] * P, CUTS[i + 1] * P
                    assert _same(out.flat[v, a:b], ref["own"][v, a:b]), f"{what}: {GNAMES[i]} of view {v}"
            if with_obj:
                assert _same(out.dobj[v], ref["dobj"][v]), f"{what}: object gradient of view {v}"
    else:
        _yard(out.flat[0], ref, P, geom, what)
        if with_obj:
            assert _same(out.dobj[0], _view_sum(ref["dobj"])), f"{what}: dobjects_dc is not ((s_0 + s_1) + s_2) + ..."
    if not with_obj:
        assert bool(torch.isnan(out.dobj).all())
    if nchunks:
        # the ranges tile [0, P) at multiples of 64, and the results are bit for bit the unchunked call's
        n = max(1, min(nchunks, (P + 63) // 64))
        assert len(seen) == n, (what, seen)
        assert [s[0] for s in seen] == list(range(n)) and seen[0][1] == 0 and seen[-1][2] == P, (what, seen)
        assert all(a[2] == b[1] for a, b in zip(seen, seen[1:])) and all(s[1] <= s[2] for s in seen), (what, seen)
        assert all(s[1] % 64 == 0 or s[1] == P for s in seen), (what, seen)
        one, _ = _call(case, mode, geom, with_go, acc, 0)
        assert _same(out.flat, one.flat), f"{what}: the 59 gradients differ from the unchunked call"
        assert _same(out.dm2, one.dm2), f"{what}: dmeans2D differs from the unchunked call"
        assert _same(out.dobj, one.dobj), f"{what}: dobjects_dc differs from the unchunked call"


def _check_layout(case):
    """What makes a view / row mix-up visible, asserted from the batch's radii (and those equal the single views')."""
    P, B = case.P, case.B
    radii = case.batch(False)[1]
    assert torch.equal(radii, _ref(case, False, False, True, False)["radii"])
    vis = radii > 0
    blind = _blind_view(B)
    seeing = [v for v in range(B) if v != blind]
    assert bool(vis[0].any())
    if P < 1000:
        return
    if blind is not None:
        assert not bool(vis[blind].any()), "the blind view sees something"
    assert bool(vis[seeing].all(dim=0).any()), "no Gaussian is seen by all seeing views"
    for v in seeing:
        others = [u for u in seeing if u != v]
        assert bool((vis[v] & ~vis[others].any(dim=0)).any()), f"view {v} sees nothing of its own"
    n64 = P // 64
    per_range = vis[:, :n64 * 64].view(B, n64, 64).any(dim=2).any(dim=0)
    assert not bool(per_range.all()), "every range of 64 Gaussians is seen by some view"
    # ... and views differ inside the chunks: every third of the scene holds Gaussians of more than one visibility pattern
    third = (P // 3 + 63) // 64 * 64
    for a in range(0, P, third):
        pat = vis[:, a:a + third].t().unique(dim=0)
        assert pat.shape[0] >= 3, f"Gaussians [{a}, {a + third}) all have the same visibility"


PB = [(63, 2), (64, 5), (65, 2), (65, 5), WIDE_PB, (1000, 2), (1000, 5), (1000, 16), (20_001, 2), (20_001, 5), (20_001, 16),
      (60_000, 2), (60_000, 5)]
BIG = 1 << 20                                       # more chunks than ceil(P / 64) for every P here
MODES = [
    ("into", dict()),
    ("into", dict(acc=True)),
    ("into", dict(nchunks=2)),
    ("into", dict(nchunks=3)),
    ("into", dict(nchunks=5)),
    ("into", dict(nchunks=BIG)),
    ("into", dict(nchunks=3, acc=True)),
    ("views", dict()),
    ("obj_into", dict(with_go=True)),
    ("obj_into", dict()),
    ("obj_views", dict(with_go=True)),
    ("obj_into", dict(with_go=True, nchunks=3)),
]


def _mode_id(m):
    return m[0] + "".join(f"-{k}{'' if v is True else v}" for k, v in m[1].items())


@pytest.mark.parametrize("P,B", PB)
def test_scene_layout_makes_views_and_chunks_differ(P, B):
    _check_layout(_case(P, B))


@pytest.mark.parametrize("geom", [True, False], ids=["geometry", "colour_only"])
@pytest.mark.parametrize("mode", MODES, ids=_mode_id)
@pytest.mark.parametrize("P,B", PB)
def test_backward_mode_writes_every_output(P, B, mode, geom):
    _check_mode(_case(P, B), mode[0], geom, **mode[1])


# ---------------------------------------------------------------------------------------------------------------------------
# the chunked cases through autograd: the path users reach (GradBucket.chunks = k, the screen-space leaf requiring grad)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_obj", [False, True], ids=["plain", "objects"])
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("P,B", [(65, 2), (1000, 5), (20_001, 16), (60_000, 5)])
def test_chunked_backward_through_autograd(P, B, k, with_obj):
    import diff_gaussian_rasterization as D
    from util import settings_for
    case = _case(P, B)
    dev, par = case.dev, case.par
    ref = _ref(case, with_obj, with_obj, True, False)
    leaves = {n: par[n].clone().requires_grad_(True) for n in ("xyz", "op", "sc", "ro")}
    dc, rest = par["dc"].clone().requires_grad_(True), par["rest"].clone().requires_grad_(True)
    obj = par["obj"].clone().requires_grad_(True) if with_obj else None
    vsp = torch.zeros(B, P, 3, device=dev, requires_grad=True)
    sts = [settings_for(c, case.bg, 3, 1.0, cls=D.GaussianRasterizationSettings, device=dev) for c in case.cams]
    bucket = D.GradBucket(P, dev)
    bucket.flat.fill_(float("nan"))
    seen = []
    bucket.chunks, bucket.on_chunk = k, (lambda c, g0, g1: seen.append((c, g0, g1)))
    res = D.rasterize_gaussians_raw_batch(leaves["xyz"], vsp, dc, rest, leaves["op"], leaves["sc"], leaves["ro"], sts,
                                          grad_bucket=bucket, objects_dc=obj)
    if with_obj:
        torch.autograd.backward([res[0], res[2]], [case.gc, case.go])
    else:
        res[0].backward(case.gc)
    torch.cuda.synchronize()
    assert torch.equal(res[1], ref["radii"])
    assert seen and seen[0][1] == 0 and seen[-1][2] == P and all(a[2] == b[1] for a, b in zip(seen, seen[1:])), seen
    assert vsp.grad is not None
    for v in range(B):
        assert _same(vsp.grad[v], ref["dm2"][v]), f"viewspace_points.grad of view {v} differs from the single-view backward"
    _yard(bucket.flat, ref, P, True, f"autograd chunks={k} P={P} B={B}")
    if with_obj:
        assert _same(obj.grad.view(P, 16), _view_sum(ref["dobj"]))


# ---------------------------------------------------------------------------------------------------------------------------
# split tiles: the boundary-record bound of a batch, and the backward with and without segments
# ---------------------------------------------------------------------------------------------------------------------------
def test_boundary_records_of_a_batch_stay_inside_their_capacity():
    """P = 60 000, B = 5: ten thousand splats of each private cluster fall on a few dozen tiles, so their lists are split
    into segments.  The forward's record count (device scalar 5) against the host's capacity bound
    N / seg + min(B * tiles_per_view, N / seg) + 1, which nothing in the kernel enforces for B > 1."""
    import diff_gaussian_rasterization as D
    case = _case(60_000, 5)
    holder, _, _, _, nren = case.batch(False)
    dv = torch.zeros(16, dtype=torch.int32, device=case.dev)
    assert case.lib.gsr_ctx_export(holder.handle, 8, ctypes.c_void_p(dv.data_ptr()), 64, case.stream()) == 0, D._err(case.lib)
    torch.cuda.synchronize()
    dv = dv.cpu().long() & 0xFFFFFFFF
    records, pairs = int(dv[5]), int(dv[0])
    assert pairs == nren == holder.info(0)
    shift = int(os.environ.get("GSR_SEG_SHIFT", "8"))
    shift = shift if 6 <= shift <= 16 else 8
    tiles = case.B * ((W + 15) // 16) * ((H + 15) // 16)
    per = pairs >> shift
    bound = per + min(tiles, per) + 1
    print(f"pairs {pairs}, boundary records {records}, bound {bound}, tiles {tiles}")
    assert records > 0, "no tile of the case is split: it does not test segments"
    assert records <= bound, (records, bound)


@pytest.mark.parametrize("geom", [True, False], ids=["geometry", "colour_only"])
def test_split_tiles_backward_equals_the_backward_without_segments(geom):
    """The same scene under GSR_FLAG_NO_SEGMENTS (whole tile lists): per-view gradients bit for bit the single-view
    backward's under the same flag (include/gsraster.h, gsr_backward_raw_batch_views); the summed ones within the yardstick
    of the single-view loop; dmeans2D bit-equal in both."""
    import diff_gaussian_rasterization as D
    seg = _case(60_000, 5)
    params, cams = _scene(60_000, 5, seed=1000 * 5 + 60_000)
    noseg = _Case(60_000, 5, seg.dev, params, cams, flags=D.FLAG_NO_SEGMENTS)
    assert torch.equal(noseg.batch(False)[2], seg.batch(False)[2]), "the images differ"
    for mode, kw in (("views", {}), ("into", {}), ("into", dict(nchunks=3))):
        _check_mode(noseg, mode, geom, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# oracle-R in float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_obj", [False, True], ids=["geometry", "objects"])
def test_chunked_batch_backward_against_the_float64_oracle(with_obj):
    """hydrant-1k, 5 views at 128x128, gsr_backward_raw_chunked with 3 ranges on the batch context (with_obj: the object
    context, given dL/dobjects): the summed gradients of every attribute group, the object features' gradient and every
    view's dmeans2D against oracle-R differentiated in float64, dL/dC (and dL/dobjects) zero on each view's fragile pixels
    on both sides.  Thresholds: those tests/test_gpu_batch.py holds the unchunked batch to -- grad_error norm <= 1e-3 and
    off-fraction <= 0.01 per group.
    The off-fraction cap is a condition of the scene, not a measurement of the kernel: oracle-R in float32 against
    oracle-R in float64 on this scene, these cameras and these seeds stays inside both thresholds for every group and every
    view's means2D (tests/test_oracle.py::test_f32_oracle_stays_inside_the_gradient_thresholds_on_the_batch_scene runs that
    on the CPU)."""
    import diff_gaussian_rasterization as D
    from gsplat_attack.scenes import make_scene
    from util import grad_error
    dev = _dev()
    model, cams, _ = make_scene("hydrant-1k", device=dev, n_views=5)
    P, B, w, h = 1000, 5, 128, 128
    params = dict(xyz=model._xyz, dc=model._features_dc, rest=model._features_rest, obj=model._objects_dc.view(P, 16),
                  op=model._opacity.view(P), sc=model._scaling, ro=model._rotation)
    case = _Case(P, B, dev, params, cams, w, h)
    gcs, gos, ref, m2, _ = oracle_batch_grads(with_obj, torch.float64)
    case.gc = torch.stack(gcs).float().to(dev).contiguous()
    case.go = torch.stack(gos).float().to(dev).contiguous()
    out, seen = _call(case, "obj_into" if with_obj else "into", True, with_obj, False, nchunks=3)
    assert len(seen) == 3
    for i, name in enumerate(GNAMES):
        norm, frac = grad_error(out.sl(i), getattr(ref, name).grad)
        print(f"{name}: norm {norm:.3e}, off {frac:.4f}")
        assert norm <= 1e-3 and frac <= 0.01, (name, norm, frac)
    if with_obj:
        norm, frac = grad_error(out.dobj[0], ref._objects_dc.grad)
        print(f"_objects_dc: norm {norm:.3e}, off {frac:.4f}")
        assert norm <= 1e-3 and frac <= 0.01, ("_objects_dc", norm, frac)
    for v in range(B):
        norm, frac = grad_error(out.dm2[v], m2[v].grad)
        print(f"dmeans2D[{v}]: norm {norm:.3e}, off {frac:.4f}")
        assert norm <= 1e-3 and frac <= 0.01, ("dmeans2D", v, norm, frac)


def oracle_batch_grads(with_obj, dtype, fragile=None):
    """oracle-R on hydrant-1k's 5 cameras, differentiated in `dtype`: -> (dL/dC per view with the fragile pixels zeroed,
    dL/dobjects likewise, the CPU model whose .grad holds the summed gradients, the views' means2D leaves, the
    views' fragile-pixel masks).
    fragile: the per-view fragile-pixel masks to use (a float32 run takes the float64 run's, so both differentiate the same
    loss); None: this run's own."""
    from gsplat_attack.scenes import make_scene
    from oracle import oracle_r as O
    from util import settings_for
    ref, rcams, _ = make_scene("hydrant-1k", device="cpu", n_views=5)
    for p_ in ref.parameters():
        p_.grad = None
    g = torch.Generator().manual_seed(31)
    gcs, gos, m2, frag = [], [], [], []
    for v in range(5):
        gc = torch.randn(3, 128, 128, generator=g).double()
        go = torch.randn(16, 128, 128, generator=g).double()
        st = settings_for(rcams[v], torch.tensor(BG))
        m2d = torch.zeros(1000, 3, dtype=dtype, requires_grad=True)
        ro = O.rasterize(ref.get_xyz, m2d, ref.get_opacity, st, shs=ref.get_features,
                         sh_objs=ref.get_objects if with_obj else None, scales=ref.get_scaling, rotations=ref.get_rotation,
                         dtype=dtype)
        solid = (~(ro.fragile_px if fragile is None else fragile[v])).double()
        gc, go = gc * solid, go * solid
        loss = (ro.color.double() * gc).sum()
        if with_obj:
            loss = loss + (ro.objects.double() * go).sum()
        loss.backward()
        gcs.append(gc); gos.append(go); m2.append(m2d); frag.append(ro.fragile_px)
    return gcs, gos, ref, m2, frag

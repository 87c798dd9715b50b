"""The library called from several host threads at once, and the workspace pool where blocks move between streams.

include/gsraster.h promises that calls on different contexts may run concurrently from different host threads; the
autograd engine relies on it (every backward and most gsr_ctx_free calls run on its thread, beside the main thread's next
forward).  Gradients are bitwise reproducible -- no float atomics -- so the reference of everything here is the SAME calls
made one after another on one stream, compared bit for bit:

  1  two threads, raw C ABI, a stream each, scenes of different block sizes       every iteration of both == serial
  2  forward on one thread, backward + free on another, one stream               every context == serial; with the
     depth / alpha maps (gsr_forward_raw_aux / gsr_ctx_set_aux_grads) as well
  3  gsr_last_error() is per thread                                               no GPU work
  4  render() + backward() from two threads (classic and fused surface, RenderCache, aux outputs)
  5  the pool under GSR_POOL_CAP_MB=1 (read once per process: tests/reentrancy_child.py): blocks last used on one
     stream are handed to another; the capped pool ends up strictly smaller than the uncapped one

Pass or fail is bit equality and byte counts, never a time.  Every join has a time limit; a thread or a child that
outlives it ends the session (no GPU work is started behind a hang)."""
import ctypes
import json
import os
import queue
import subprocess
import sys
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

JOIN_S = 60.0
ITERS = 20
CUTS = (0, 3, 6, 51, 52, 55, 59)                   # xyz | f_dc | f_rest | opacity | scaling | rotation (GradBucket's layout)
GNAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
NAN = float("nan")


def _D():
    import diff_gaussian_rasterization as D
    D._load()
    return D


def _q(t):
    return ctypes.c_void_p(None) if t is None else ctypes.c_void_p(t.data_ptr())


def _same(a, b):
    """Bit-equal, NaN patterns included (a float nobody wrote must still be the NaN it was filled with)."""
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _start(fns):
    """One daemon thread per callable; what a thread raises is kept for the caller."""
    errs = []

    def wrap(fn):
        def run():
            try:
                fn()
            except BaseException as e:                # noqa: BLE001 -- reported by _join
                errs.append(e)
        return run
    threads = [threading.Thread(target=wrap(fn), daemon=True) for fn in fns]
    for t in threads:
        t.start()
    return threads, errs


def _join(threads, errs):
    for t in threads:
        t.join(JOIN_S)
    if any(t.is_alive() for t in threads):
        pytest.exit(f"test_gpu_reentrancy: a thread did not finish within {JOIN_S:.0f} s; no more GPU work is started", 1)
    if errs:
        raise errs[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the raw C ABI: one view of one model, its output buffers, the three calls
# ---------------------------------------------------------------------------------------------------------------------------
class _View:
    def __init__(self, D, model, cam, bg, dev, seed):
        from gsplat_attack.renderer import PipelineParams, _settings
        self.dev, self.P = dev, int(model._xyz.shape[0])
        self.H, self.W = int(cam.image_height), int(cam.image_width)
        self.pack = D._SettingsPack(_settings(cam, model, PipelineParams(), bg, 1.0), dev)
        self.par = [t.detach().contiguous() for t in (model._xyz, model._features_dc, model._features_rest, model._opacity,
                                                      model._scaling, model._rotation)]
        g = torch.Generator().manual_seed(seed)
        self.gc = torch.randn(3, self.H, self.W, generator=g).to(dev)
        self.gd = torch.randn(self.H, self.W, generator=g).to(dev)          # dL/ddepth, dL/dalpha of the aux variant
        self.ga = torch.randn(self.H, self.W, generator=g).to(dev)


class _Bufs:
    """What one forward + backward writes: image, radii, the 59 attribute gradients (one flat bucket), dmeans2D, and the
    two maps of an _aux forward."""
    KEYS = ("color", "radii", "flat", "dm2", "depth", "alpha")

    def __init__(self, v, fill):
        dev = v.dev
        self.color = torch.full((3, v.H, v.W), NAN, device=dev)
        self.radii = torch.full((v.P,), -1, dtype=torch.int32, device=dev)
        self.flat = torch.full((59 * v.P,), fill, device=dev)
        self.dm2 = torch.full((v.P, 3), NAN, device=dev)
        self.depth = torch.full((v.H, v.W), NAN, device=dev)
        self.alpha = torch.full((v.H, v.W), NAN, device=dev)

    def reset(self, fill):
        self.color.fill_(NAN); self.radii.fill_(-1); self.flat.fill_(fill); self.dm2.fill_(NAN)
        self.depth.fill_(NAN); self.alpha.fill_(NAN)

    def items(self):
        return [(k, getattr(self, k)) for k in self.KEYS]


def _forward(D, lib, v, b, st, aux=False):
    xyz, dc, rest, op, sc, ro = v.par
    handle, nren = ctypes.c_void_p(None), ctypes.c_int64(0)
    head = (ctypes.byref(v.pack.c), v.P, _q(xyz), _q(dc), _q(rest), None, _q(op), _q(sc), _q(ro), _q(b.color), None,
            _q(b.radii), ctypes.byref(handle), ctypes.byref(nren))
    if aux:
        rc = lib.gsr_forward_raw_aux(*head, _q(b.depth), _q(b.alpha), st)
    else:
        rc = lib.gsr_forward_raw(*head, st)
    assert rc == 0 and handle.value, D._err(lib)
    return handle.value


def _backward(D, lib, v, h, b, st, accumulate, aux=False):
    h = ctypes.c_void_p(h)
    if aux:
        assert lib.gsr_ctx_set_aux_grads(h, _q(v.gd), _q(v.ga)) == 0, D._err(lib)
    s = [b.flat[CUTS[i] * v.P:CUTS[i + 1] * v.P] for i in range(6)]
    rc = lib.gsr_backward_raw_into(h, _q(v.gc), None, _q(s[0]), _q(b.dm2), _q(s[1]), _q(s[2]), None, _q(s[3]), _q(s[4]),
                                   _q(s[5]), accumulate, st)
    assert rc == 0, D._err(lib)


def _scenes(dev):
    """-> (hydrant-1k model, its 2 cameras, hydrant-full model at 30000 Gaussians / 320x240, its cameras, background)."""
    from gsplat_attack.scenes import make_scene
    small, cams_s, _ = make_scene("hydrant-1k", device=dev, n_views=2)
    big, cams_b, _ = make_scene("hydrant-full", device=dev, P=30000, width=320, height=240, n_views=6)
    return small, cams_s, big, cams_b, torch.tensor([0.1, 0.2, 0.3], device=dev)


def _pool_bytes(lib):
    out = ctypes.c_int64(0)
    assert lib.gsr_query(1, ctypes.byref(out)) == 0
    return out.value


# ---------------------------------------------------------------------------------------------------------------------------
# 1. two threads, a stream each
# ---------------------------------------------------------------------------------------------------------------------------
def _sequence(D, lib, v, s, n, start=None, hook=None):
    """n x (gsr_forward_raw -> gsr_backward_raw_into, adding into zeroed buffers -> gsr_ctx_free) of one view on stream s;
    every iteration's buffers are copied, on s, into row i of the returned tensors."""
    with torch.cuda.stream(s):
        b = _Bufs(v, 0.0)
        snap = {k: torch.empty((n,) + tuple(t.shape), dtype=t.dtype, device=v.dev) for k, t in b.items()}
        st = ctypes.c_void_p(s.cuda_stream)
        if start is not None:
            start.wait(JOIN_S)
        for i in range(n):
            b.reset(0.0)
            h = _forward(D, lib, v, b, st)
            _backward(D, lib, v, h, b, st, 1)
            lib.gsr_ctx_free(ctypes.c_void_p(h))
            for k, t in b.items():
                snap[k][i].copy_(t)
            if hook is not None:
                hook(i)
    return snap


def test_two_threads_on_their_own_streams_equal_the_serial_sequences():
    """Thread 0: 20 x forward / backward / free of hydrant-1k view 0; thread 1: the same on hydrant-full view 0 (other block
    sizes: the pool's best-fit search sees foreign blocks); both released by one barrier.  Image, radii, the six gradient
    tensors and dmeans2D of EVERY iteration of both threads equal the serial run on the default stream, and the pool holds
    after iteration 20 what it held after iteration 5 (both threads stand at a barrier while it is read)."""
    D = _D()
    lib = D._load()
    dev = torch.device("cuda:0")
    small, cams_s, big, cams_b, bg = _scenes(dev)
    views = [_View(D, small, cams_s[0], bg, dev, 11), _View(D, big, cams_b[0], bg, dev, 12)]
    ref = [_sequence(D, lib, v, torch.cuda.current_stream(dev), ITERS) for v in views]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in views]
    go, mid = threading.Barrier(2), threading.Barrier(2)
    got, pool_mid = [None, None], []

    def worker(t):
        def hook(i):
            if i == 4:                               # after iteration 5: both threads stand still while the pool is read
                try:
                    mid.wait(JOIN_S)
                    if t == 0:
                        pool_mid.append(_pool_bytes(lib))
                    mid.wait(JOIN_S)
                except threading.BrokenBarrierError:
                    raise RuntimeError("the other thread did not reach iteration 5")

        def run():
            try:
                got[t] = _sequence(D, lib, views[t], streams[t], ITERS, start=go, hook=hook)
            except BaseException:
                go.abort(); mid.abort()
                raise
        return run
    threads, errs = _start([worker(0), worker(1)])
    _join(threads, errs)
    torch.cuda.synchronize()
    pool_end = _pool_bytes(lib)
    compared = 0
    for t in range(2):
        # the serial reference repeats itself: what every iteration is held to is one value per buffer
        for k in ("color", "radii", "flat", "dm2"):
            for i in range(ITERS):
                assert _same(ref[t][k][i], ref[t][k][0]), (t, k, i, "serial run not reproducible")
                assert _same(got[t][k][i], ref[t][k][i]), (t, k, i)
        for i in range(ITERS):
            for j, name in enumerate(GNAMES):
                a = got[t]["flat"][i, CUTS[j] * views[t].P:CUTS[j + 1] * views[t].P]
                assert bool(torch.isfinite(a).all()), (t, name, i)
            compared += 1
        assert float(ref[t]["flat"][0].abs().max()) > 0 and int(ref[t]["radii"][0].max()) > 0
    assert pool_mid
    print(f"two threads: {compared} iterations compared, pool {pool_mid[0]} bytes after iteration 5, {pool_end} after 20")
    assert pool_end == pool_mid[0]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. forward on one thread, backward and free on another (the autograd engine's pattern)
# ---------------------------------------------------------------------------------------------------------------------------
def _serial_contexts(D, lib, views, n, aux):
    st = ctypes.c_void_p(torch.cuda.current_stream(views[0].dev).cuda_stream)
    out = []
    for k in range(n):
        v = views[k % len(views)]
        b = _Bufs(v, NAN)
        h = _forward(D, lib, v, b, st, aux)
        _backward(D, lib, v, h, b, st, 0, aux)
        lib.gsr_ctx_free(ctypes.c_void_p(h))
        out.append(b)
    torch.cuda.synchronize()
    return out


AUX_FORWARDS = 2000                                # per thread; 2 maps x 64 KB a call (hydrant-1k is 128 x 128)


def _aux_forwards_from_two_threads(D, lib, views, refs):
    """Thread t: AUX_FORWARDS x (gsr_forward_raw_aux -> gsr_ctx_free) of views[t] on a stream of its own, call i writing
    its maps into slice i -> how many slices of either thread differ from refs[t]'s maps (bit for bit)."""
    dev, n = views[0].dev, AUX_FORWARDS
    maps = [{k: torch.full((n, v.H, v.W), NAN, device=dev) for k in ("depth", "alpha")} for v in views]
    scratch = [_Bufs(v, NAN) for v in views]
    streams = [torch.cuda.Stream(device=dev) for _ in views]
    torch.cuda.synchronize()
    go = threading.Barrier(len(views))

    def worker(t):
        def run():
            v, b, st = views[t], scratch[t], ctypes.c_void_p(streams[t].cuda_stream)
            xyz, dc, rest, op, sc, ro = v.par
            handle, nren = ctypes.c_void_p(None), ctypes.c_int64(0)
            try:
                go.wait(JOIN_S)
                for i in range(n):
                    rc = lib.gsr_forward_raw_aux(ctypes.byref(v.pack.c), v.P, _q(xyz), _q(dc), _q(rest), None, _q(op), _q(sc),
                                                 _q(ro), _q(b.color), None, _q(b.radii), ctypes.byref(handle),
                                                 ctypes.byref(nren), _q(maps[t]["depth"][i]), _q(maps[t]["alpha"][i]), st)
                    assert rc == 0 and handle.value, D._err(lib)
                    lib.gsr_ctx_free(handle)
            except BaseException:
                go.abort()
                raise
        return run
    threads, errs = _start([worker(t) for t in range(len(views))])
    _join(threads, errs)
    torch.cuda.synchronize()
    wrong = 0
    for t in range(len(views)):
        ok = torch.ones(n, dtype=torch.bool, device=dev)
        for k in ("depth", "alpha"):
            want = getattr(refs[t], k).view(torch.int32)
            ok &= (maps[t][k].view(torch.int32) == want).flatten(1).all(1)
        wrong += int((~ok).sum())
    return wrong


@pytest.mark.parametrize("aux", [False, True])
def test_forward_on_one_thread_backward_and_free_on_another(aux):
    """Thread A issues forwards on stream S and hands (handle, buffers) over a queue of two; thread B differentiates
    (overwriting NaN-filled buffers) and frees on S while A is already in the next forward.  20 contexts, alternating the
    two hydrant-1k views, each bit-equal to the serial loop.
    aux: A calls gsr_forward_raw_aux, B arms gsr_ctx_set_aux_grads; the maps land in the caller's buffers and the armed
    backward equals the serial one.  The _aux entry points pass their two pointers to the forward through a per-thread
    slot that only a forward takes (and clears), and B never runs one: a slot shared by all threads would go unnoticed
    with A and B alone.  So the variant goes on with AUX_FORWARDS forward-only _aux calls (each freed at once) from each of
    two threads, a stream and a view each, every call writing its maps into a slice of its own: with a shared slot a
    forward that gets between another's store and its read takes those pointers, and a slice stays NaN or holds the other
    view's map.  The window is a few instructions at the head of a call of some hundred microseconds, hence the count."""
    D = _D()
    lib = D._load()
    dev = torch.device("cuda:0")
    small, cams_s, _, _, bg = _scenes(dev)
    views = [_View(D, small, cams_s[i], bg, dev, 21 + i) for i in range(2)]
    ref = _serial_contexts(D, lib, views, ITERS, aux)
    bufs = [_Bufs(views[k % 2], NAN) for k in range(ITERS)]
    S = torch.cuda.Stream(device=dev)
    S.wait_stream(torch.cuda.current_stream(dev))
    st = ctypes.c_void_p(S.cuda_stream)
    q = queue.Queue(maxsize=2)

    def thread_a():
        try:
            for k in range(ITERS):
                q.put((_forward(D, lib, views[k % 2], bufs[k], st, aux), k), timeout=JOIN_S)
        finally:
            q.put(None, timeout=JOIN_S)

    def thread_b():
        while True:
            item = q.get(timeout=JOIN_S)
            if item is None:
                return
            h, k = item
            _backward(D, lib, views[k % 2], h, bufs[k], st, 0, aux)
            lib.gsr_ctx_free(ctypes.c_void_p(h))

    threads, errs = _start([thread_a, thread_b])
    _join(threads, errs)
    torch.cuda.synchronize()
    keys = _Bufs.KEYS if aux else _Bufs.KEYS[:4]
    for k in range(ITERS):
        for name in keys:
            assert _same(getattr(bufs[k], name), getattr(ref[k], name)), (k, name)
        assert bool(torch.isfinite(bufs[k].flat).all()) and bool(torch.isfinite(bufs[k].dm2).all()), k
        if aux:
            assert bool(torch.isfinite(bufs[k].depth).all()) and bool(torch.isfinite(bufs[k].alpha).all()), k
            assert float(bufs[k].alpha.max()) > 0
    if aux:
        # the armed backward is not the plain one: the maps' gradients reached the geometry
        plain = _serial_contexts(D, lib, views, 1, False)[0]
        assert not _same(plain.flat, ref[0].flat)
        wrong = _aux_forwards_from_two_threads(D, lib, views, [ref[0], ref[1]])
        print(f"aux variant: {ITERS} contexts compared; {2 * AUX_FORWARDS} forward-only calls, {wrong} with a wrong map")
        assert wrong == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. gsr_last_error() is per thread
# ---------------------------------------------------------------------------------------------------------------------------
def test_error_text_is_per_thread():
    """x: gsr_knn_dist2(P=-1); y: gsr_query(99) -- argument checks, no launch.  Order: x refused, y refused, x reads (must
    see its own text although y's is newer), x refused again, y reads (must see its own although x's is newer)."""
    D = _D()
    lib = D._load()
    lib.gsr_knn_dist2.restype = ctypes.c_int
    lib.gsr_knn_dist2.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    e1, e2, e3 = threading.Event(), threading.Event(), threading.Event()
    seen = {}

    def x():
        assert lib.gsr_knn_dist2(None, -1, None, None) == 1
        e1.set()
        assert e2.wait(JOIN_S)
        seen["x"] = bytes(lib.gsr_last_error())
        assert lib.gsr_knn_dist2(None, -1, None, None) == 1
        e3.set()

    def y():
        assert e1.wait(JOIN_S)
        out = ctypes.c_int64(0)
        assert lib.gsr_query(99, ctypes.byref(out)) == 1
        e2.set()
        assert e3.wait(JOIN_S)
        seen["y"] = bytes(lib.gsr_last_error())
    threads, errs = _start([x, y])
    _join(threads, errs)
    assert seen["x"].startswith(b"gsr_knn_dist2"), seen
    assert seen["y"].startswith(b"gsr_query: unknown item 99"), seen


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the Python surface from two threads
# ---------------------------------------------------------------------------------------------------------------------------
def _render_loop(model, cam, pipe, bg, gc, s, n, start=None):
    """n x (render -> backward(gc)) of one camera under stream s -> per iteration (image, radii, grads, depth, alpha)."""
    from gsplat_attack.renderer import render
    out = []
    with torch.cuda.stream(s):
        if start is not None:
            start.wait(JOIN_S)
        for _ in range(n):
            model.zero_grad()
            r = render(cam, model, pipe, bg)
            r["render"].backward(gc)
            out.append((r["render"].detach().clone(), r["radii"].clone(),
                        {k: getattr(model, k).grad.detach().clone() for k in GNAMES},
                        r["render_depth"].detach().clone() if "render_depth" in r else None,
                        r["render_alpha"].detach().clone() if "render_alpha" in r else None))
            del r
    return out


def test_render_and_backward_from_two_threads():
    """Thread 0: the classic surface (activated tensors through `rasterize`) with the depth / alpha maps; thread 1: the fused
    raw path through a RenderCache (nine of its ten renders are re-renders of the kept context).  Both render the SAME
    camera object -- the binding's cache of dense camera tensors is shared between the threads' streams -- each on its own
    model.clone() under its own stream, ten iterations.  Images, maps, radii and every .grad equal the serial runs; the
    process-wide flags are what they were."""
    D = _D()
    from gsplat_attack.renderer import PipelineParams
    dev = torch.device("cuda:0")
    _, _, big, cams_b, bg = _scenes(dev)
    cam, n = cams_b[0], 10
    gc = torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(31)).to(dev)
    flags = D._FLAGS

    def pipes():
        return [PipelineParams(skip_objects=True, fused_activations=False, aux_outputs=True),
                PipelineParams(skip_objects=True, render_cache=D.RenderCache())]
    ref = [_render_loop(big.clone(), cam, p, bg, gc, torch.cuda.current_stream(dev), n) for p in pipes()]
    torch.cuda.synchronize()
    models, ps = [big.clone(), big.clone()], pipes()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    go, got = threading.Barrier(2), [None, None]

    def worker(t):
        def run():
            try:
                got[t] = _render_loop(models[t], cam, ps[t], bg, gc, streams[t], n, start=go)
            except BaseException:
                go.abort()
                raise
        return run
    threads, errs = _start([worker(0), worker(1)])
    _join(threads, errs)
    torch.cuda.synchronize()
    assert D._FLAGS == flags
    assert ps[1].render_cache.hits == n - 1 and ps[1].render_cache.misses == 1
    for t in range(2):
        for i in range(n):
            img0, rad0, g0, d0, a0 = ref[t][i]
            img1, rad1, g1, d1, a1 = got[t][i]
            assert torch.equal(img0, img1), (t, i, "image")
            assert torch.equal(rad0, rad1), (t, i, "radii")
            for k in GNAMES:
                assert torch.equal(g0[k], g1[k]), (t, i, k)
            assert (d0 is None) == (d1 is None) == (t == 1)
            if d0 is not None:
                assert torch.equal(d0, d1) and torch.equal(a0, a1), (t, i, "maps")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the pool under pressure: cross-stream block reuse (a child process per setting of GSR_POOL_CAP_MB)
# ---------------------------------------------------------------------------------------------------------------------------
def _child(mode, cap_mb):
    env = dict(os.environ)
    env.pop("GSR_POOL_CAP_MB", None)
    if cap_mb is not None:
        env["GSR_POOL_CAP_MB"] = str(cap_mb)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reentrancy_child.py")
    try:
        p = subprocess.run([sys.executable, script, mode], env=env, timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.exit(f"test_gpu_reentrancy: the {mode} child did not finish within 120 s; no more GPU work is started", 1)
    if p.returncode < 0:
        pytest.exit(f"test_gpu_reentrancy: the {mode} child was ended by signal {-p.returncode}; no more GPU work is "
                    f"started\n{p.stderr[-2000:]}", 1)
    assert p.returncode == 0, f"{mode} child failed\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def test_pool_under_pressure_hands_blocks_across_streams():
    """tests/reentrancy_child.py twice, one child at a time: with GSR_POOL_CAP_MB=1 (every request beyond the first MB takes
    a fitting free block of another stream, behind a wait for that stream) and without.  Both: every equality true.  Capped:
    the pool stops growing after the second round over the stream ring, holds strictly less than the uncapped pool -- where
    each of the three streams keeps blocks of its own; the proof that the cross-stream path ran -- and no less than a
    serial view needs."""
    capped = _child("capped", 1)
    free = _child("uncapped", None)
    print("capped  ", json.dumps(capped))
    print("uncapped", json.dumps(free))
    for r, cap in ((capped, 1), (free, None)):
        assert r["cap_mb"] == cap
        assert r["equal"] and all(r["equal"].values()), r["equal"]
        assert r["rounds"] == 4 and len(r["pool_after_round"]) == 4
        assert r["trim"]["after"] <= r["trim"]["before"] and r["trim"]["after_backward"] <= r["trim"]["before"], r["trim"]
        assert r["trim"]["after"] >= r["ctx_bytes"] > 0
    after = capped["pool_after_round"]
    assert after[3] == after[1], after
    assert after[3] < free["pool_after_round"][3], (after, free["pool_after_round"])
    # what the first serial view left in an empty pool: every block it needs, so no less than the largest of them
    assert after[3] >= capped["serial_view_bytes"] >= capped["ctx_bytes"], (after, capped["serial_view_bytes"])

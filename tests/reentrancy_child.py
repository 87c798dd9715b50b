"""Child process of tests/test_gpu_reentrancy.py::test_pool_under_pressure_hands_blocks_across_streams: the workspace pool
under the GSR_POOL_CAP_MB of its environment (read once per process).  argv[1] names the mode ("capped" / "uncapped": a
label, the cap itself comes from the environment).  On hydrant-full at 30000 Gaussians, 320x240, 6 views:

  a  the serial per-view loop on one stream                                          the reference
  b  StreamRing(3) over the 6 views, 4 rounds                                        every round == a, bit for bit
  c  one render_batch of the 6 views, then one view on a ring stream                 == the same calls on one stream
  d  the colour attack with kept contexts (pgd_attack, cache_binning), 3 streams     == the attack on 1 stream: history,
                                                                                      success flags, parameters, saved bytes
  e  trim_pool() while one context is alive                                          its backward gives a's bits

Prints one JSON line; exits non-zero when an equality is false."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

ROUNDS = 4


def _grads(model, names):
    return {n: getattr(model, n).grad.detach().clone() for n in names}


def _eq(a, b):
    """(image, radii, grads) against (image, radii, grads), bit for bit."""
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and set(a[2]) == set(b[2])
                and all(torch.equal(a[2][n], b[2][n]) for n in a[2]))


def main(mode):
    import diff_gaussian_rasterization as D
    from gsplat_attack import dist as gdist
    from gsplat_attack.renderer import PipelineParams, render, render_batch
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.streams import StreamRing
    names = gdist.ATTACK_PARAMS
    dev = torch.device("cuda:0")
    W, H, V = 320, 240, 6
    model, cams, _ = make_scene("hydrant-full", device=dev, P=30000, width=W, height=H, n_views=V)
    pipe = PipelineParams(skip_objects=True)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    gcs = [torch.randn(3, H, W, generator=torch.Generator().manual_seed(10 + i)).to(dev) for i in range(V)]
    cap = os.environ.get("GSR_POOL_CAP_MB")
    res = dict(mode=mode, cap_mb=int(cap) if cap else None, rounds=ROUNDS, equal={})
    equal = res["equal"]

    def view(i, keep=False):
        model.zero_grad()
        out = render(cams[i], model, pipe, bg)
        if keep:
            return out
        out["render"].backward(gcs[i])
        return out["render"].detach().clone(), out["radii"].clone(), _grads(model, names)

    # ---- a: the serial loop, from an empty pool ----------------------------------------------------------------------
    torch.cuda.synchronize()
    D.trim_pool()
    res["pool_at_start"] = D.pool_bytes()
    ref, ctx_bytes = [], 0
    for i in range(V):
        model.zero_grad()
        out = render(cams[i], model, pipe, bg)
        if i == 0:
            ctx_bytes = out["render"].grad_fn.holder.info(2)     # the two blocks view 0's context holds on to
        out["render"].backward(gcs[i])
        ref.append((out["render"].detach().clone(), out["radii"].clone(), _grads(model, names)))
        if i == 0:
            res["serial_view_bytes"] = D.pool_bytes()
    del out
    torch.cuda.synchronize()
    res["ctx_bytes"] = int(ctx_bytes)
    res["pool_after_serial"] = D.pool_bytes()

    # ---- b: the stream ring ------------------------------------------------------------------------------------------
    ring = StreamRing(3, dev)
    res["pool_after_round"] = []
    for rnd in range(ROUNDS):
        got = []
        for i in range(V):
            with ring.next():
                got.append(view(i))
        ring.join()
        torch.cuda.synchronize()
        equal[f"b_round{rnd + 1}"] = all(_eq(r, g) for r, g in zip(ref, got))
        res["pool_after_round"].append(D.pool_bytes())

    # ---- c: a batch on the caller's stream, then one view on a ring stream -------------------------------------------
    gc_all = torch.stack(gcs)

    def batch_then_view(on_ring):
        model.zero_grad()
        rb = render_batch(cams, model, pipe, bg)
        rb["render"].backward(gc_all)
        first = (rb["render"].detach().clone(), rb["radii"].clone(), _grads(model, names))
        del rb
        if on_ring:
            with ring.next():
                second = view(2)
            ring.join()
        else:
            second = view(2)
        torch.cuda.synchronize()
        return first, second
    one = batch_then_view(False)
    two = batch_then_view(True)
    equal["c_batch"] = _eq(one[0], two[0])
    equal["c_view_after_batch"] = _eq(one[1], two[1]) and _eq(ref[2], two[1])
    res["pool_after_batch"] = D.pool_bytes()

    # ---- d: kept contexts re-rendered and differentiated on ring streams (pool_retag) -------------------------------
    # The colour attack of tests/test_gpu_rerender.py on THIS scene and its 6 views.  The single-stream run never takes a
    # block of another stream: it is the reference of the 3-stream run (and cache off, on 3 streams, of cache on).
    from gsplat_attack.attack import pgd_attack
    COL = ("_features_dc", "_features_rest")
    back = model.clone()

    def attack(streams, cache_on, tmp):
        m = model.clone()
        calls, recs = [], []

        def success(im, i):
            calls.append(float(im.double().sum()))
            return len(calls) > 3 * V                 # fooled from the fourth iteration on
        path = os.path.join(tmp, f"m_{streams}_{cache_on}.ply")
        hist = pgd_attack(m, cams, iters=6, groups=("color",), streams=streams, success_fn=success, background=back,
                          log=recs.append, save_path=path, cache_binning=cache_on, batched=False)
        torch.cuda.synchronize()
        with open(path, "rb") as f:
            saved = f.read()
        return hist, [r.get("successes") for r in recs], calls, {n: getattr(m, n).detach().clone() for n in COL}, saved

    def same_run(a, b):
        (h0, f0, c0, p0, s0), (h1, f1, c1, p1, s1) = a, b
        return bool(len(h0) == 4 and h0 == h1 and f0 == f1 and c0 == c1 and s0 == s1
                    and all(torch.equal(p0[n], p1[n]) for n in COL))
    with tempfile.TemporaryDirectory() as tmp:
        one_stream = attack(1, True, tmp)
        three_streams = attack(3, True, tmp)
        three_plain = attack(3, False, tmp)
    equal["d_streams3_vs_streams1"] = same_run(one_stream, three_streams)
    equal["d_cache_on_vs_off"] = same_run(three_plain, three_streams)
    res["d_iterations"] = len(three_streams[0])
    res["pool_after_attack"] = D.pool_bytes()
    del one_stream, three_streams, three_plain
    torch.cuda.synchronize()

    # ---- e: trim_pool() under a live context -------------------------------------------------------------------------
    out = view(0, keep=True)
    torch.cuda.synchronize()
    before = D.pool_bytes()
    D.trim_pool()
    after = D.pool_bytes()
    out["render"].backward(gcs[0])
    torch.cuda.synchronize()
    equal["e_backward_after_trim"] = _eq(ref[0], (out["render"].detach(), out["radii"], _grads(model, names)))
    res["trim"] = dict(before=before, after=after, after_backward=D.pool_bytes())
    del out

    print(json.dumps(res))
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "uncapped"))

"""The 16 object channels through the batched launch chain (render_batch(objects=True), gsr_*_batch_obj*).

The yardstick of every check is the per-view path: render() with object channels (PipelineParams(skip_objects=False)) on
each camera, and -- for gradients -- its backward passes accumulated in view order.  Images, radii and object maps are bit
for bit those of the single view; the object features' gradient is bit for bit the accumulated .grad of the loop (the batch
forms every view's sum as the single view does and adds them in view order); the 59 attribute gradients meet the
double-sum yardstick of tests/test_gpu_batch.py (the batch's fused per-Gaussian kernel sums the views in another
association).  One view per small scene is also held against oracle-R."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _loop(model, cams, bg, gcs, gos, pipe=None):
    """The reference's loop: render() with objects + backward per view.  -> images, radii, object maps, screen-space
    gradients, the accumulated 59-float bucket, the views' buckets summed in double, the accumulated object gradient and
    every view's own object gradient."""
    import diff_gaussian_rasterization as D
    from gsplat_attack.renderer import PipelineParams, render
    P = int(model.get_xyz.shape[0])
    dev = model.get_xyz.device
    pipe = copy.copy(pipe or PipelineParams(skip_objects=False))
    bucket, own = D.GradBucket(P, dev), D.GradBucket(P, dev)
    pipe_own = copy.copy(pipe)
    pipe.grad_bucket, pipe_own.grad_bucket = bucket, own
    exact = torch.zeros(59 * P, dtype=torch.float64, device=dev)
    imgs, radii, objs, vs, own_obj = [], [], [], [], []
    model._objects_dc.grad = None
    for v, cam in enumerate(cams):
        out = render(cam, model, pipe, bg)
        torch.autograd.backward([out["render"], out["render_object"]], [gcs[v], gos[v]])
        imgs.append(out["render"].detach())
        radii.append(out["radii"])
        objs.append(out["render_object"].detach())
        vs.append(out["viewspace_points"].grad.clone())
    acc_obj = model._objects_dc.grad.clone()
    for v, cam in enumerate(cams):
        own.reset()
        model._objects_dc.grad = None
        out = render(cam, model, pipe_own, bg)
        torch.autograd.backward([out["render"], out["render_object"]], [gcs[v], gos[v]])
        exact += own.flat.double()
        own_obj.append(model._objects_dc.grad.clone())
    model._objects_dc.grad = None
    return dict(render=torch.stack(imgs), radii=torch.stack(radii), objects=torch.stack(objs), vs=vs, bucket=bucket,
                exact=exact, obj_grad=acc_obj, own_obj=own_obj)


def _batch(model, cams, bg, gcs, gos, pipe=None):
    import diff_gaussian_rasterization as D
    from gsplat_attack.renderer import PipelineParams, render_batch
    P = int(model.get_xyz.shape[0])
    bucket = D.GradBucket(P, model.get_xyz.device)
    pipe = copy.copy(pipe or PipelineParams())
    if pipe.grad_bucket is None:
        pipe.grad_bucket = bucket
    model._objects_dc.grad = None
    out = render_batch(cams, model, pipe, bg, objects=True)
    grads = [torch.stack(list(gcs))] + ([torch.stack(list(gos))] if gos is not None else [])
    torch.autograd.backward([out["render"]] + ([out["render_object"]] if gos is not None else []), grads)
    g_obj = model._objects_dc.grad.clone()
    model._objects_dc.grad = None
    return out, bucket, g_obj


def _yardstick(loop_bucket, exact, batch_bucket):
    """tests/test_gpu_batch.py's double-sum yardstick for the 59 attribute gradients."""
    P = loop_bucket.P
    for name, s1, s2, c0, c1 in zip(loop_bucket.NAMES, loop_bucket.slices(), batch_bucket.slices(), loop_bucket.CUTS[:-1],
                                    loop_bucket.CUTS[1:]):
        ex = exact[c0 * P:c1 * P]
        scale_ = ex.abs().max().item()
        e_seq = (s1.double() - ex).abs().max().item()
        e_bat = (s2.double() - ex).abs().max().item()
        floor = 1e-4 if name in ("_scaling", "_rotation") else 1e-5
        assert e_bat <= max(3.0 * e_seq, floor * scale_), f"{name}: batch {e_bat:.3e}, loop {e_seq:.3e}, scale {scale_:.3e}"


def _rand(shape, n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g).to(dev) for _ in range(n)]


def _check(model, cams, seed):
    dev = model.get_xyz.device
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    bg = torch.tensor(BG, device=dev)
    gcs, gos = _rand((3, H, W), len(cams), seed, dev), _rand((16, H, W), len(cams), seed + 1, dev)
    ref = _loop(model, cams, bg, gcs, gos)
    out, bucket, g_obj = _batch(model, cams, bg, gcs, gos)
    torch.cuda.synchronize()
    assert out["render_object"].shape == (len(cams), 16, H, W)
    assert torch.equal(out["render"].detach(), ref["render"]), "batched images differ from the single views"
    assert torch.equal(out["radii"], ref["radii"])
    assert torch.equal(out["render_object"].detach(), ref["objects"]), "batched object maps differ from the single views"
    for v in range(len(cams)):
        assert torch.equal(out["viewspace_points"].grad[v], ref["vs"][v]), f"view {v}: screen-space gradient differs"
    assert torch.equal(g_obj, ref["obj_grad"]), "object-feature gradient differs from the loop's accumulated .grad"
    _yardstick(ref["bucket"], ref["exact"], bucket)
    return out


def test_small_scene_objects_bit_equal_and_oracle():
    """S-hydrant-1k at 128^2, B = 3; view 1's object map and its object-feature gradient against oracle-R (float64)."""
    from gsplat_attack.scenes import make_scene
    from oracle import oracle_r as O
    from util import grad_error, model_inputs, settings_for
    dev = _dev()
    model, cams, _ = make_scene("hydrant-1k", device=dev, n_views=3)
    out = _check(model, cams, 3)
    ref, rcams, _ = make_scene("hydrant-1k", device="cpu", n_views=3)
    st = settings_for(rcams[1], torch.tensor(BG))
    gc, go = _rand((3, 128, 128), 1, 7, "cpu")[0], _rand((16, 128, 128), 1, 8, "cpu")[0]
    ro, rg = O.forward_backward(model_inputs(ref), st, gc, go, drop_fragile=True)
    solid = ~ro.fragile_px
    err = (out["render_object"][1].detach().cpu().double() - ro.objects.detach()).abs().amax(dim=0)[solid].max().item()
    assert err <= 1e-4, err
    # view 1's dL/d object features: a batch whose dL/dC and dL/dobjects are zero on the other views
    gcs_s, gos_s = O.solid_grads(ro, gc, go)
    z3, z16 = torch.zeros(3, 128, 128, device=dev), torch.zeros(16, 128, 128, device=dev)
    _, _, g_obj = _batch(model, cams, torch.tensor(BG, device=dev), [z3, gcs_s.float().to(dev), z3],
                         [z16, gos_s.float().to(dev), z16])
    norm, frac = grad_error(g_obj, rg["sh_objs"])
    assert norm <= 1e-3 and frac <= 0.01, (norm, frac)


@pytest.mark.parametrize("P,W,H,B", [(60_000, 640, 360, 5), (20_001, 333, 190, 3), (70_000, 512, 512, 16)])
def test_mid_scenes_objects_bit_equal(P, W, H, B):
    """Counts and sizes that are no multiple of anything, up to the largest batch."""
    from gsplat_attack.scenes import make_scene
    dev = _dev()
    model, cams, _ = make_scene("nyc-1M", device=dev, P=P, width=W, height=H, n_views=B)
    _check(model, cams, P)


def test_backward_without_object_gradient_is_the_no_object_batch():
    """The attack's case: an object forward whose map is not differentiated.  The backward is the segmented no-object
    composite: every gradient bit for bit the no-object batch's, the object features' gradient zero."""
    import diff_gaussian_rasterization as D
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.renderer import PipelineParams, render_batch
    dev = _dev()
    model, cams, _ = make_scene("nyc-1M", device=dev, P=60_000, width=640, height=360, n_views=4)
    bg = torch.tensor(BG, device=dev)
    gcs = _rand((3, 360, 640), 4, 21, dev)
    out, b_obj, g_obj = _batch(model, cams, bg, gcs, None)
    P = int(model.get_xyz.shape[0])
    b_plain = D.GradBucket(P, dev)
    plain = render_batch(cams, model, PipelineParams(skip_objects=True, grad_bucket=b_plain), bg)
    plain["render"].backward(torch.stack(gcs))
    torch.cuda.synchronize()
    assert torch.equal(out["render"].detach(), plain["render"].detach())
    assert torch.equal(b_obj.flat, b_plain.flat)
    assert torch.equal(out["viewspace_points"].grad, plain["viewspace_points"].grad)
    assert not bool(g_obj.any())


def test_per_view_object_gradients():
    """gsr_backward_raw_batch_obj_views: every view's object gradient and 59-float bucket bit for bit that view's
    single-view backward; through a GradBucketSet the binding hands autograd their view-ordered sum."""
    import diff_gaussian_rasterization as D
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.renderer import PipelineParams, render_batch
    dev = _dev()
    B, W, H = 4, 480, 272
    model, cams, _ = make_scene("nyc-1M", device=dev, P=40_000, width=W, height=H, n_views=B)
    P = int(model.get_xyz.shape[0])
    bg = torch.tensor(BG, device=dev)
    gcs, gos = _rand((3, H, W), B, 31, dev), _rand((16, H, W), B, 32, dev)
    ref = _loop(model, cams, bg, gcs, gos)
    # the C entry point on a kept batch context
    out = render_batch(cams, model, PipelineParams(), bg, objects=True)
    lib = D._load()
    bset = D.GradBucketSet(B, P, dev)
    dobj = torch.full((B, P, 16), float("nan"), device=dev)
    d_m2 = torch.empty(B, P, 3, device=dev)
    gc, go = torch.stack(gcs).contiguous(), torch.stack(gos).contiguous()
    sl = bset.bucket(0).slices()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.gsr_backward_raw_batch_obj_views(out["render"].grad_fn.holder.handle, gc.data_ptr(), go.data_ptr(),
                                              sl[0].data_ptr(), d_m2.data_ptr(), sl[1].data_ptr(), sl[2].data_ptr(),
                                              dobj.data_ptr(), sl[3].data_ptr(), sl[4].data_ptr(), sl[5].data_ptr(), 59 * P,
                                              stream)
    assert rc == 0, D._err(lib)
    torch.cuda.synchronize()
    own = D.GradBucket(P, dev)
    pipe_own = PipelineParams(skip_objects=False, grad_bucket=own)
    from gsplat_attack.renderer import render
    for v in range(B):
        assert torch.equal(dobj[v], ref["own_obj"][v].view(P, 16)), f"view {v}: object gradient differs"
        own.reset()
        o = render(cams[v], model, pipe_own, bg)
        torch.autograd.backward([o["render"], o["render_object"]], [gcs[v], gos[v]])
        torch.cuda.synchronize()
        assert torch.equal(bset.bucket(v).flat, own.flat), f"view {v}: attribute gradients differ"
        assert torch.equal(d_m2[v], ref["vs"][v])
    model._objects_dc.grad = None
    del out
    # through autograd with a GradBucketSet: the view-ordered sum
    _, _, g_obj = _batch(model, cams, bg, gcs, gos, pipe=PipelineParams(grad_bucket=D.GradBucketSet(B, P, dev)))
    assert torch.equal(g_obj, ref["obj_grad"])


def test_kept_batch_context_rerenders_objects():
    """RenderCache: a colour step, then the kept batch context re-rendered (gsr_ctx_rerender with out_objects [B,16,H,W]);
    image, object map and the backward after it bit for bit a fresh render_batch(objects=True)."""
    import diff_gaussian_rasterization as D
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.renderer import PipelineParams
    dev = _dev()
    B, W, H = 3, 320, 200
    model, cams, _ = make_scene("nyc-1M", device=dev, P=30_000, width=W, height=H, n_views=B)
    bg = torch.tensor(BG, device=dev)
    gcs, gos = _rand((3, H, W), B, 41, dev), _rand((16, H, W), B, 42, dev)
    cache = D.RenderCache()
    pipe = PipelineParams(render_cache=cache)
    _batch(model, cams, bg, gcs, gos, pipe=pipe)                       # first render: the context is kept
    with torch.no_grad():
        model._features_dc.add_(0.05)
    hits = cache.hits
    out_c, b_c, g_c = _batch(model, cams, bg, gcs, gos, pipe=pipe)     # re-render of the kept context
    assert cache.hits == hits + 1
    out_f, b_f, g_f = _batch(model, cams, bg, gcs, gos)                # fresh
    torch.cuda.synchronize()
    assert torch.equal(out_c["render"].detach(), out_f["render"].detach())
    assert torch.equal(out_c["render_object"].detach(), out_f["render_object"].detach())
    assert torch.equal(b_c.flat, b_f.flat) and torch.equal(g_c, g_f)
    assert torch.equal(out_c["viewspace_points"].grad, out_f["viewspace_points"].grad)


def test_pair_batch_objects_equal_render_pair():
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.renderer import PipelineParams, render_pair, render_pair_batch
    dev = _dev()
    a, cams, _ = make_scene("nyc-1M", device=dev, P=20_001, width=333, height=190, n_views=3)
    b, _, _ = make_scene("hydrant-1k", device=dev)
    bg = torch.tensor(BG, device=dev)
    pipe = PipelineParams(skip_objects=False)
    out = render_pair_batch(cams, a, b, pipe, bg, objects=True)
    assert out["render_object"].shape == (3, 16, 190, 333)
    for v, c in enumerate(cams):
        r = render_pair(c, a, b, pipe, bg)
        assert torch.equal(out["render"][v], r["render"]), v
        assert torch.equal(out["radii"][v], r["radii"]), v
        assert torch.equal(out["render_object"][v], r["render_object"]), v


def test_render_views_crosses_batch_limit_and_sizes():
    """20 cameras: 18 at 128^2 then 2 at 96x64 -> batches of 16, 2 and 2; every dict bit for bit render()'s."""
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.renderer import PipelineParams, render, render_views
    dev = _dev()
    model, cams, _ = make_scene("hydrant-1k", device=dev, n_views=18)
    _, cams2, _ = make_scene("hydrant-1k", device=dev, n_views=2, width=96, height=64)
    allc = cams + cams2
    bg = torch.tensor(BG, device=dev)
    pipe = PipelineParams(skip_objects=False)
    outs = render_views(allc, model, pipe, bg)
    assert len(outs) == 20
    with torch.no_grad():
        for c, o in zip(allc, outs):
            r = render(c, model, pipe, bg)
            assert torch.equal(o["render"], r["render"]) and torch.equal(o["radii"], r["radii"])
            assert torch.equal(o["render_object"], r["render_object"])
            assert torch.equal(o["visibility_filter"], r["visibility_filter"])
            assert o["viewspace_points"].shape == r["viewspace_points"].shape


def test_objects_need_object_features():
    from gsplat_attack.scenes import make_scene
    from gsplat_attack.renderer import PipelineParams, can_batch, render_batch
    from gsplat_attack.gaussian_model import GaussianModel
    dev = _dev()
    model, cams, _ = make_scene("hydrant-1k", device=dev, n_views=2)
    assert can_batch(cams, model, PipelineParams(), objects=True)
    assert not can_batch(cams, model, PipelineParams())
    bare = GaussianModel.from_tensors(xyz=model._xyz.detach(), features_dc=model._features_dc.detach(),
                                      features_rest=model._features_rest.detach(), scaling=model._scaling.detach(),
                                      rotation=model._rotation.detach(), opacity=model._opacity.detach(),
                                      objects_dc=torch.zeros(0, 1, 16, device=dev), device=dev)
    with pytest.raises(ValueError):
        render_batch(cams, bare, PipelineParams(), torch.zeros(3, device=dev), objects=True)


def test_fullsize_batch_of_four_objects():
    """S-nyc-1M at 1080p, B = 4: 32 640 tiles, the one-wave-per-tile object compositor in a batch."""
    from gsplat_attack.scenes import make_scene
    dev = _dev()
    model, cams, _ = make_scene("nyc-1M", device=dev, n_views=8)
    _check(model, [cams[i] for i in (0, 3, 5, 6)], 99)

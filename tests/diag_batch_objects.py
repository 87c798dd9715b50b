"""Diagnostic: the object channels through the batched launch chain against one render() per view, alternated in one
process on one stream, S-nyc-1M at 1080p with the scene's eight ring cameras.  Views/s of
  (a) forward only with object maps: a render() loop against render_views (batches of up to 8 here: the eight cameras);
  (b) forward + backward without dL/dobjects (the attack's case) at B = 5 and 8: object forward, backward of the image;
  (c) forward + backward with dL/dobjects at B = 5 and 8.
python tests/diag_batch_objects.py [reps] [rounds]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import diff_gaussian_rasterization as D  # noqa: E402
from gsplat_attack.renderer import PipelineParams, render, render_batch, render_views  # noqa: E402
from gsplat_attack.scenes import make_scene  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device("cuda:0")
    model, cams, spec = make_scene("nyc-1M", device=dev, n_views=8)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    P = int(model.get_xyz.shape[0])
    bg = torch.zeros(3, device=dev)
    g = torch.Generator().manual_seed(99)
    gc = torch.randn(3, H, W, generator=g).to(dev)
    go = torch.randn(16, H, W, generator=g).to(dev)
    bucket = D.GradBucket(P, dev)
    pipe = PipelineParams(skip_objects=False, grad_bucket=bucket)
    pipe_b = PipelineParams(grad_bucket=bucket)

    def loop_fwd(cs):
        with torch.no_grad():
            for c in cs:
                render(c, model, pipe, bg)

    def batch_fwd(cs):
        render_views(cs, model, pipe, bg, max_batch=len(cs))

    def loop_bwd(cs, with_go):
        bucket.reset()
        model._objects_dc.grad = None
        for c in cs:
            out = render(c, model, pipe, bg)
            if with_go:
                torch.autograd.backward([out["render"], out["render_object"]], [gc, go])
            else:
                out["render"].backward(gc)

    def batch_bwd(cs, with_go):
        bucket.reset()
        model._objects_dc.grad = None
        B = len(cs)
        out = render_batch(cs, model, pipe_b, bg, objects=True)
        gcb = gc.unsqueeze(0).expand(B, 3, H, W)
        if with_go:
            torch.autograd.backward([out["render"], out["render_object"]], [gcb, go.unsqueeze(0).expand(B, 16, H, W)])
        else:
            out["render"].backward(gcb)

    cases = [("a fwd+objects", 8, lambda cs: loop_fwd(cs), lambda cs: batch_fwd(cs))]
    for B in (5, 8):
        cases.append(("b fwd+bwd no dL/dobj", B, lambda cs: loop_bwd(cs, False), lambda cs: batch_bwd(cs, False)))
    for B in (5, 8):
        cases.append(("c fwd+bwd with dL/dobj", B, lambda cs: loop_bwd(cs, True), lambda cs: batch_bwd(cs, True)))
    print(f"{spec.name} P={P} {W}x{H}, {reps} reps x {rounds} alternating rounds, median per form", flush=True)
    for name, B, loop_fn, batch_fn in cases:
        cs = cams[:B]
        for fn in (loop_fn, batch_fn):
            for _ in range(2):
                fn(cs)
        torch.cuda.synchronize()
        ts = {"loop": [], "batch": []}
        for _ in range(rounds):
            for form, fn in (("loop", loop_fn), ("batch", batch_fn)):
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn(cs)
                torch.cuda.synchronize()
                ts[form].append((time.perf_counter() - t0) / reps)
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        vl, vb = B / med["loop"], B / med["batch"]
        print(f"{name:24s} B={B:2d}: loop {vl:8.1f} views/s, batch {vb:8.1f} views/s, batch/loop {vb / vl:5.3f}", flush=True)


if __name__ == "__main__":
    main()

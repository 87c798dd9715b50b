"""Diagnostic (not collected by pytest): the detector-input stage, HIP against the torch composition it replaces, on
one device in one process.  B = 8 renders of 3 x 1080 x 1920 -> letterbox 640 x 640, forward + backward through autograd,
timed with device events after a warm-up, the two variants alternating; then the backward kernel on its own, for its
achieved bandwidth (bytes the algorithm needs: grad_src written once, the resized rectangle of grad_dst read once).

    python tests/diag_detector_input.py [--B 8] [--height 1080] [--width 1920] [--size 640] [--iters 500] [--rounds 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.nn.functional as F


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diag_detector_input: needs a HIP device (no CPU timing is meaningful)")
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import image_ops as IO
    from gsplat_attack import detector_input as DI
    D._load()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(args.B, 3, args.height, args.width, device=dev, generator=gen).requires_grad_(True)
    new = (args.size, args.size)
    scale, rh, rw, top, left = DI.letterbox_geometry(args.height, args.width, new)
    g = torch.randn(args.B, 3, *new, device=dev, generator=gen)
    pads = (left, new[1] - left - rw, top, new[0] - top - rh)

    def hip():
        x.grad = None
        DI.letterbox(x, new)[0].backward(g)

    def torch_ops():
        x.grad = None
        F.pad(F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False), pads, value=114 / 255).backward(g)

    spec = IO.ResampleSpec(new[0], new[1], rh, rw, top, left, 114 / 255)
    out = torch.empty_like(x)

    def hip_bwd_only():
        IO.resample_backward(g, spec, x.shape, out=out)

    def hip_fwd_only():
        with torch.no_grad():
            DI.letterbox(x, new)

    fns = {"hip_fwd_bwd_ms": hip, "torch_fwd_bwd_ms": torch_ops, "hip_bwd_kernel_ms": hip_bwd_only, "hip_fwd_kernel_ms": hip_fwd_only}
    for fn in fns.values():                       # warm-up: code objects, the allocator's blocks, autograd's buffers
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    hip()
    g_hip = x.grad.clone()
    torch_ops()
    res = {"B": args.B, "src": [args.height, args.width], "dst": list(new), "resized": [rh, rw],
           "max_abs_grad_diff_vs_torch": float((g_hip - x.grad).abs().max())}
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):                  # alternate the variants: other work shares the host
        for k, fn in fns.items():
            runs[k].append(timed(fn, args.iters))
    for k, v in runs.items():
        res[k] = min(v)
        res[k + "_all"] = [round(t, 4) for t in v]
    bytes_bwd = 4 * args.B * 3 * (args.height * args.width + rh * rw)
    res["hip_bwd_bytes"] = bytes_bwd
    res["hip_bwd_GBps"] = bytes_bwd / (res["hip_bwd_kernel_ms"] * 1e-3) / 1e9
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Diagnostic (not collected by pytest): the set-prediction detector stage, HIP against what a user does without it -- the
float32 oracle of tests/setdet_cases.py as torch ops on the device, its match on the host (scipy's linear_sum_assignment if
scipy imports, else the oracle's own matcher; either way one device-to-host copy of the cost matrix per call) and autograd
-- at DETR's own shape (B = 8, Q = 100, C = 91, one gt row per image) and at Q = 900 with 8 rows.  Times come from device
events after a warm-up, the variants alternating; a report, not an acceptance criterion.

    python tests/diag_set_detector.py [--iters 50] [--rounds 3] [--out profiles/set_detector_times.txt]
    python tests/diag_set_detector.py --hip-only --iters 50          # only the library's calls: under a kernel profiler
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import setdet_cases as SC
    from diff_gaussian_rasterization import setdet_ops as SO

    try:
        from scipy.optimize import linear_sum_assignment

        def solver(cost, rows):
            r2c = np.full(cost.shape[0], -1, np.int64)
            ri, ci = linear_sum_assignment(cost[rows])
            r2c[np.asarray(rows)[ri]] = ci
            return r2c, float(cost[rows][ri, ci].sum())
        how = "scipy.optimize.linear_sum_assignment"
    except ImportError:
        solver, how = None, "the oracle's own matcher"

    dev = torch.device("cuda:0")
    spec = SO.SetDetSpec(img_w=SC.FRAME[0], img_h=SC.FRAME[1])
    lines = []
    for c in (SC.Case("detr", 8, 100, 91, 1), SC.Case("detr-900", 8, 900, 91, 8)):
        x, bx, gb, gc = (torch.tensor(a).to(dev) for a in SC.make_inputs(c))

        def hip():
            return SO.run(x, bx, gb, gc, spec, want_grad=True, want_matching=False)

        def hip_forward():
            return SO.run(x, bx, gb, gc, spec, want_grad=False, want_matching=False)

        def hip_post():
            return SO.postprocess(x, bx, spec)

        def torch_ops():
            return SC.oracle(x, bx, gb, gc, torch.float32, device=dev, solver=solver)

        if args.hip_only:
            for _ in range(args.iters):
                hip()
                hip_post()
            torch.cuda.synchronize()
            continue
        loss = hip()[0]
        o = torch_ops()
        torch.cuda.synchronize()
        lines.append(f"set-prediction detector stage, B={c.B} Q={c.Q} C={c.C} M={c.M}: loss {[round(v, 6) for v in loss.tolist()]}, "
                     f"torch float32 on the device {[round(v, 6) for v in o['loss'].tolist()]}")
        fns = dict(hip=hip, hip_forward=hip_forward, hip_post=hip_post, torch=torch_ops)
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        best = {k: 1e9 for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                best[k] = min(best[k], timed(torch, fn, args.iters))
        lines.append(f"  HIP, loss + gradients  {best['hip']:.4f} ms")
        lines.append(f"  HIP, loss only         {best['hip_forward']:.4f} ms")
        lines.append(f"  HIP, postprocess       {best['hip_post']:.4f} ms")
        lines.append(f"  torch device ops       {best['torch']:.4f} ms  (float32 oracle, match on the host by {how}, autograd backward)")
    if args.hip_only:
        return
    lines.append("  (wall time per call including the Python binding and the workspace allocation; best of "
                 f"{args.rounds} rounds of {args.iters} calls)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

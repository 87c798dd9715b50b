"""Diagnostic (not collected by pytest): the detector loss stage, HIP against the same contract written in torch device
ops (the float32 oracle of tests/detloss_cases.py run on the device, forward + autograd backward), at the reference's own
shape: 640 x 640, A = 8400, C = 80, one gt row per image, B = 8.  Times come from device events after a warm-up, the two
variants alternating; a report, not an acceptance criterion.

    python tests/diag_detector_loss.py [--iters 50] [--rounds 3] [--batch 8] [--out profiles/detector_loss_times.txt]
    python tests/diag_detector_loss.py --hip-only --iters 50          # only the library's calls: under a kernel profiler
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    import torch
    import detloss_cases as DC
    from diff_gaussian_rasterization import detloss_ops as LO

    dev = torch.device("cuda:0")
    c = DC.BY_ID["full"]._replace(B=args.batch)
    pred, gtb, gtc = (torch.tensor(a).to(dev) for a in DC.make_inputs(c))
    levels = c.levels

    def hip():
        return LO.run(pred, levels, gtb, gtc, want_grad=True, want_assignment=False)

    def hip_forward():
        return LO.run(pred, levels, gtb, gtc, want_grad=False, want_assignment=False)

    def torch_ops():
        return DC.oracle(levels, pred, gtb, gtc, torch.float32, device=dev)

    if args.hip_only:
        for _ in range(args.iters):
            hip()
        torch.cuda.synchronize()
        return
    loss = hip()[0]
    o = torch_ops()
    torch.cuda.synchronize()
    lines = [f"detector loss stage, B={c.B} A={c.A} C={c.C} M={c.M}: loss {[round(v, 6) for v in loss.tolist()]}, "
             f"torch float32 on the device {[round(v, 6) for v in o['loss'].tolist()]}"]
    for fn in (hip, hip_forward, torch_ops):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    best = {"hip": 1e9, "hip_forward": 1e9, "torch": 1e9}
    for _ in range(args.rounds):
        best["hip"] = min(best["hip"], timed(torch, hip, args.iters))
        best["hip_forward"] = min(best["hip_forward"], timed(torch, hip_forward, args.iters))
        best["torch"] = min(best["torch"], timed(torch, torch_ops, max(args.iters // 10, 3)))
    nbytes = c.B * c.A * (2 * c.C + 64 + 64) * 4              # logits read, gradient written, the bins of the decode read
    lines.append(f"  HIP, loss + gradient   {best['hip']:.4f} ms  ({nbytes / best['hip'] / 1e9:.3f} TB/s of the tensors it must touch)")
    lines.append(f"  HIP, loss only         {best['hip_forward']:.4f} ms")
    lines.append(f"  torch device ops       {best['torch']:.4f} ms  (float32 oracle, forward + autograd backward)")
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

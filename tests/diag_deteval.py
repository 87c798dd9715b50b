"""Diagnostic (not collected by pytest): the detection metrics at COCO's working size on one device -- 400 images x 100 detections x
80 classes, 8 ground-truth rows per image, COCO's 10 IoU thresholds, 4 area ranges, caps (1, 10, 100) and 101 recall thresholds.

  (a) match        gsr_deteval_match over the 400 images as one batch (one launch, one workgroup per image)
  (b) accumulate   gsr_deteval_accumulate over its outputs (two radix sorts, a scan, one wave per (class, area, cap, threshold))
  (c) summarize    gsr_deteval_summarize (one launch)
  (d) all three through the binding, allocations of the outputs and the workspace included
  (e) the NumPy oracle of tests/deteval_cases.py on the same arrays on this host's CPU, once (plain Python loops: the kind of
      evaluator the stage replaces; pycocotools is not a dependency, so it is not measured), and the host build of the kernels'
      header (tests/host_math/deteval_host.cpp: the same arithmetic in C++ loops on one thread), once

(a)-(d) are medians of `--iters` samples timed with device events on an idle stream after a warm-up: end-to-end times of a call,
the Python / ctypes path in front of the launches included, not kernel times.  The GPU results are compared with the oracle's bit
for bit and the outcome is printed.  A report of what was seen, not an acceptance criterion.

    python tests/diag_deteval.py [--iters 30] [--images 400] [--out profiles/deteval_times.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

D, K, M = 100, 80, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--images", type=int, default=400)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import deteval_cases as DC
    from diff_gaussian_rasterization import deteval_ops as EO

    N = args.images
    rng = np.random.default_rng(7)
    dets, counts, gt, gt_cls = DC._scene(rng, N, D, M, K, rng.integers(60, D + 1, N), big=True)
    spec = DC.Spec(K, D, M)
    es = EO.EvalSpec(K, tuple(spec.iou.tolist()), spec.areas, spec.caps, spec.R)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    d, c, g, k, rec = t(dets), t(counts), t(gt), t(gt_cls), t(spec.rec)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    m = EO.match(d, c, g, k, es)
    acc = EO.accumulate(d, m, k, rec, es)

    def all_three():
        mm = EO.match(d, c, g, k, es)
        ac = EO.accumulate(d, mm, k, rec, es)
        return mm, ac, EO.summarize(ac[0], ac[2], es)
    steps = {"match": lambda: EO.match(d, c, g, k, es), "accumulate": lambda: EO.accumulate(d, m, k, rec, es),
             "summarize": lambda: EO.summarize(acc[0], acc[2], es), "all three": all_three}
    for fn in steps.values():                                                # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in steps}
    for _ in range(args.iters):                                              # the variants take turns
        for n, fn in steps.items():
            samples[n].append(timed(fn)[0])
    mm, ac, stats = all_three()
    torch.cuda.synchronize()
    live = int((m.dt_order >= 0).sum())
    lines = [f"detection metrics: {N} images x {D} detections ({live} live) x {K} classes, {M} gt rows per image, T=10 A=4 caps (1, 10, 100) R=101",
             f"device {torch.cuda.get_device_name(0)}; medians of {args.iters} samples (min .. max), device events, idle stream, ms per call"]
    for n, v in samples.items():
        lines.append(f"  {n:<11s} {statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})")
    if not args.no_oracle:
        t0 = time.perf_counter()
        ref = DC.oracle_run(spec, [(dets, counts, gt, gt_cls)])
        cpu_s = time.perf_counter() - t0
        got = dict(zip(EO.MatchOut._fields, mm))
        got.update(precision=ac[0], scores=ac[1], recall=ac[2], npig=ac[3], stats=stats)
        try:
            DC.check("diag", got, ref)
            verdict = "every output equal to the oracle's, doubles bit for bit"
        except AssertionError as e:
            verdict = f"DIFFERS from the oracle: {e}"
        lines.append(f"  NumPy oracle on this host's CPU (one run, one thread of Python loops): {cpu_s:8.2f} s")
        t0 = time.perf_counter()
        DC.host_run(spec, [(dets, counts, gt, gt_cls)])
        lines.append(f"  host build of csrc/gsr_deteval.h on this host's CPU (one run, one thread, g++ -O1): {time.perf_counter() - t0:8.3f} s")
        lines.append(f"  {verdict}")
        lines.append("  " + "  ".join(f"{n} {v:.4f}" for n, v in zip(DC.STAT_NAMES, ref["stats"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

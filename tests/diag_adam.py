"""Diagnostic (not collected by pytest): the fused Adam step at a working size, P = 1 000 000 Gaussians with the model's seven
shapes (75 floats per Gaussian, 28 bytes moved per float), in one run on one device:

  (a) gsr_adam_step_multi over the seven tensors: one launch
  (b) torch.optim.Adam (default: foreach) on the same parameters and gradients
  (c) torch.optim.Adam(fused=True), if this torch build constructs it
  (d) (a) with a row range that leaves the last 1 % of the rows live (the inpaint shape)
  (e) (a) with a row mask of a random 1 % of the rows

Two figures per variant, both medians of `--iters` samples timed with device events after a warm-up, the variants taking
turns: "single" is one step enqueued on an idle stream -- event, call, event -- and so includes the Python and ctypes time in
front of the launch (an end-to-end latency, not a kernel time); "queued" is `--batch` steps between the two events divided by
their number, where the device works behind the host and the figure is the larger of the kernel time and the host's time
per call.  The achieved bytes per second is 28 B x elements / the queued time, beside the 6.3 TB/s a float4 copy reaches on
this chip.  Kernel times proper come from a kernel trace of this script in a run of its own.  The kernel's registers, scratch
and occupancy are in csrc/README.md's kernel table (csrc/resusage.sh prints them).  A report, not an acceptance criterion.

    python tests/diag_adam.py [--iters 50] [--batch 20] [--out profiles/adam_times.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

P = 1_000_000
SHAPES = ((P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4), (P, 1, 16))
LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001, 0.0025)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from diff_gaussian_rasterization import adam_ops

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    xs = [torch.randn(s, device=dev, generator=g) for s in SHAPES]
    gs = [torch.randn(s, device=dev, generator=g) for s in SHAPES]
    ms = [torch.zeros_like(x) for x in xs]
    vs = [torch.zeros_like(x) for x in xs]
    items = list(zip(xs, gs, ms, vs))
    elements = sum(x.numel() for x in xs)
    count = [0]
    rand_mask = (torch.rand(P, device=dev, generator=g) < 0.01).to(torch.uint8)

    def fused(row_mask=None, rows=None):
        count[0] += 1
        assert adam_ops.adam_step_(items, count[0], list(LRS), (0.9, 0.999), 1e-15, row_mask, rows)

    params = [torch.nn.Parameter(x.clone()) for x in xs]
    for p, gr in zip(params, gs):
        p.grad = gr
    groups = lambda: [dict(params=[p], lr=lr) for p, lr in zip(params, LRS)]   # noqa: E731
    variants = {"fused step (gsr_adam_step_multi)": fused,
                "torch.optim.Adam (foreach)": torch.optim.Adam(groups(), lr=0.0, eps=1e-15).step}
    notes = []
    try:
        variants["torch.optim.Adam(fused=True)"] = torch.optim.Adam(groups(), lr=0.0, eps=1e-15, fused=True).step
    except Exception as e:   # noqa: BLE001
        notes.append(f"torch.optim.Adam(fused=True) could not be constructed by this torch build: {e}")
    variants["fused step, last 1 % of rows live (range)"] = lambda: fused(rows=(P - P // 100, P))
    variants["fused step, random 1 % of rows live (mask)"] = lambda: fused(row_mask=rand_mask)

    # the same result first: one step of (a) against one step of torch on copies
    chk = [torch.nn.Parameter(x.clone()) for x in xs]
    for p, gr in zip(chk, gs):
        p.grad = gr
    torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(chk, LRS)], lr=0.0, eps=1e-15).step()
    fused()
    worst = max(float((x - p.detach()).abs().max()) for x, p in zip(xs, chk))
    notes.append(f"one step from zero state, fused against torch.optim.Adam on the device: largest |difference| {worst:.3e}")
    del chk

    times = {k: [] for k in variants}
    queued = {k: [] for k in variants}
    for k, fn in variants.items():                     # warm-up: code objects, torch's state tensors
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.iters):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    for _ in range(args.iters):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.batch):
                fn()
            b.record()
            b.synchronize()
            queued[k].append(a.elapsed_time(b) / args.batch)
    lines = [f"Adam step at P = {P} (seven tensors, {elements} floats, {28 * elements / 1e9:.2f} GB moved by a full step); "
             f"medians of {args.iters} samples, device events, variants in turn; {torch.cuda.get_device_name(0)}",
             f"  single = one step on an idle stream (includes the host's time in front of the launch); queued = {args.batch} steps "
             "between the events, per step"]
    for k, ts in times.items():
        med, q = statistics.median(ts), statistics.median(queued[k])
        line = f"  {k:48s} single {med:8.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})   queued {q:8.4f} ms (min {min(queued[k]):.4f})"
        if k.startswith("fused step (") or k.startswith("torch"):
            line += f"  {28 * elements / (q * 1e-3) / 1e12:.2f} TB/s of 6.3"
        lines.append(line)
    lines += notes
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Diagnostic (not collected by pytest): the fused image losses (gsr_imgloss) at a working size -- B = 8 views, C = 3,
1920 x 1080 -- with and without a gradient, against the reference's _ssim restated in torch on the device (the 11 x 11
window as five depthwise convolutions) with and without its autograd backward.  Both sides compute 1 - ssim per image; the
values are compared first (printed, not asserted).  Times come from device events after a warm-up, the variants
alternating.  A report, not an acceptance criterion.

    python tests/diag_imgloss.py [--iters 3] [--rounds 3] [--out profiles/imgloss_times.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, C, H, W = 8, 3, 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from diag_roi_detector import timed
    from diff_gaussian_rasterization import imgloss_ops as IL
    from diff_gaussian_rasterization._ops_common import workspace_bytes

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    y = torch.rand((B, C, H, W), generator=g).to(dev)
    x = (y + 0.1 * torch.randn((B, C, H, W), generator=g).to(dev)).contiguous()
    spec = IL.ImgLossSpec(0.0, 0.0, 1.0)
    from math import exp
    taps = torch.tensor([exp(-(k - 5) ** 2 / 4.5) for k in range(11)], dtype=torch.float32)
    taps = taps / taps.sum()
    win = (taps[:, None] @ taps[None, :]).expand(C, 1, 11, 11).contiguous().to(dev)

    def torch_ssim(a, b):
        mu1, mu2 = F.conv2d(a, win, padding=5, groups=C), F.conv2d(b, win, padding=5, groups=C)
        mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = F.conv2d(a * a, win, padding=5, groups=C) - mu1_sq
        s2 = F.conv2d(b * b, win, padding=5, groups=C) - mu2_sq
        s12 = F.conv2d(a * b, win, padding=5, groups=C) - mu12
        m = ((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
        return m.mean(dim=(1, 2, 3))

    def hip_fwd():
        return IL.imgloss_forward(x, y, spec, want_grad=False)[0]

    def hip_grad():
        return IL.imgloss_forward(x, y, spec, want_grad=True)

    def torch_fwd():
        with torch.no_grad():
            return 1 - torch_ssim(x, y)

    def torch_grad():
        a = x.detach().requires_grad_(True)
        (1 - torch_ssim(a, y)).sum().backward()
        return a.grad

    n = B * C * H * W
    full = workspace_bytes("gsr_imgloss_workspace_bytes", IL.c_spec(spec, x.shape))
    small = workspace_bytes("gsr_imgloss_workspace_bytes", IL.c_spec(spec, x.shape, IL.NO_GRAD))
    lines = [f"fused image losses at B={B} C={C} {W}x{H} ({n * 4 / 1e6:.0f} MB per image tensor), tile {IL.TILE[0]}x{IL.TILE[1]}; "
             f"workspace {full / 1e6:.0f} MB with a gradient (the three derivative maps), {small / 1e6:.2f} MB without"]
    print(lines[0], flush=True)
    t_hip, g_hip, _ = hip_grad()
    t_ref, g_ref = torch_fwd(), torch_grad()
    torch.cuda.synchronize()
    print("  warm-up done", flush=True)
    lines.append(f"  1 - ssim per image, largest difference from the torch restatement: {(t_hip[:, 3] - t_ref).abs().max().item():.3e}; "
                 f"gradient: {(g_hip - g_ref).abs().max().item():.3e} of {g_ref.abs().max().item():.3e}")
    again = hip_grad()
    lines.append(f"  second call bit-equal: terms {torch.equal(again[0], t_hip)}, gradient {torch.equal(again[1], g_hip)}; "
                 f"terms without a gradient bit-equal {torch.equal(hip_fwd(), t_hip)}")
    fns = dict(hip_fwd=hip_fwd, torch_fwd=torch_fwd, hip_grad=hip_grad, torch_grad=torch_grad)
    best = {k: 1e9 for k in fns}
    for r in range(args.rounds):
        for k, fn in fns.items():
            best[k] = min(best[k], timed(torch, fn, args.iters))
        print(f"  round {r} done", flush=True)
    # bytes the kernels must move: the tile pass reads 2 n floats (+ halo) and, with a gradient, writes 3 n; the gradient pass
    # reads 3 n (+ halo) + 2 n and writes n
    lines.append(f"  terms only,    gsr_imgloss (two launches)                 {best['hip_fwd']:.3f} ms   "
                 f"({2 * n * 4 / best['hip_fwd'] / 1e6:.0f} GB/s of the 2 n floats read)")
    lines.append(f"  terms only,    torch: five depthwise 11x11 convolutions   {best['torch_fwd']:.3f} ms   "
                 f"(fused / torch = {best['hip_fwd'] / best['torch_fwd']:.3f})")
    lines.append(f"  with gradient, gsr_imgloss (three launches)               {best['hip_grad']:.3f} ms   "
                 f"({11 * n * 4 / best['hip_grad'] / 1e6:.0f} GB/s of the 11 n floats read and written)")
    lines.append(f"  with gradient, torch: the same + autograd                 {best['torch_grad']:.3f} ms   "
                 f"(fused / torch = {best['hip_grad'] / best['torch_grad']:.3f})")
    lines.append(f"  (device events, best of {args.rounds} rounds of {args.iters} calls; the times include the Python binding and the output "
                 "allocations on both sides)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

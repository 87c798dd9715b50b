"""Diagnostic (not collected by pytest): gsr_roi_align and gsr_roi_align_backward at the reference detector's working size
(B = 5 views, Cf = 1024, a 50 x 68 stride-16 map, S = 512 RoIs per image, 14 x 14 bins: about 2 GB of pooled output)
against a torch-ops restatement of the same computation on the same device -- F.grid_sample (border padding, which equals
the stage's read for RoIs inside the image) and a 2 x 2 average for the forward, its autograd backward, which scatters with
float atomics, for the backward.  Both sides use sampling_ratio = 2; the adaptive grid the reference runs is timed for the
HIP side alone.  Times come from device events after a warm-up, the variants alternating.  Also printed: how many of an
image's RoIs a tile of the backward actually walks (the workgroup-uniform cull), and the forward's share of the measured
HBM store rate.  A report, not an acceptance criterion.

    python tests/diag_roi_detector.py [--iters 5] [--rounds 3] [--out profiles/roi_detector_times.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, CF, HF, WF, S, P, STRIDE = 5, 1024, 50, 68, 512, 14, 16
HBM_STORE_TBS = 6.1          # plain dword stores as measured on an MI355X


def timed(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def make_rois(np, rs):
    """Proposals as an RPN clipped to the image leaves them: widths and heights from 32 px to most of the image."""
    W, H = WF * STRIDE, HF * STRIDE
    w = np.exp(rs.uniform(np.log(32.0), np.log(0.9 * W), (B, S)))
    h = np.exp(rs.uniform(np.log(32.0), np.log(0.9 * H), (B, S)))
    x1, y1 = rs.uniform(0, 1, (B, S)) * (W - w), rs.uniform(0, 1, (B, S)) * (H - h)
    return np.stack([x1, y1, x1 + w, y1 + h], -1).astype(np.float32)


def tile_counts(np, rois, tile=8):
    """RoIs per (image, tile) that pass the backward's span test (csrc/gsr_rcnn.hip.h, span_misses)."""
    lo = rois[..., :2] / STRIDE - 0.5
    hi = rois[..., 2:] / STRIDE - 0.5
    out = []
    for y0 in range(0, HF, tile):
        for x0 in range(0, WF, tile):
            hit = (hi[..., 1] >= y0 - 2) & (lo[..., 1] <= y0 + tile + 1) & (hi[..., 0] >= x0 - 2) & (lo[..., 0] <= x0 + tile + 1)
            out.append(hit.sum(1))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from diff_gaussian_rasterization import rcnn_ops as RO

    dev = torch.device("cuda:0")
    rs = np.random.RandomState(3)
    rois_np = make_rois(np, rs)
    rois = torch.tensor(rois_np).to(dev)
    feat = torch.randn((B, CF, HF, WF), generator=torch.Generator().manual_seed(4)).to(dev)
    spec2 = RO.RcnnSpec(PH=P, PW=P, spatial_scale=1.0 / STRIDE, sampling_ratio=2)
    spec0 = spec2._replace(sampling_ratio=0)
    gp = torch.randn((B, S, CF, P, P), device=dev)
    gf = torch.empty_like(feat)

    def torch_grid():
        sx, sy = rois[..., 0] / STRIDE - 0.5, rois[..., 1] / STRIDE - 0.5
        bx, by = (rois[..., 2] - rois[..., 0]) / STRIDE / P, (rois[..., 3] - rois[..., 1]) / STRIDE / P
        k = (torch.arange(2 * P, device=dev) // 2).float() + ((torch.arange(2 * P, device=dev) % 2).float() + 0.5) / 2
        xs, ys = sx[..., None] + k * bx[..., None], sy[..., None] + k * by[..., None]            # [B,S,28]
        gx = (2 * xs / (WF - 1) - 1)[:, :, None, :].expand(B, S, 2 * P, 2 * P)
        gy = (2 * ys / (HF - 1) - 1)[:, :, :, None].expand(B, S, 2 * P, 2 * P)
        return torch.stack([gx, gy], -1).reshape(B, S * 2 * P, 2 * P, 2)

    grid = torch_grid()

    def torch_forward(f=feat):
        out = []
        for b in range(B):
            v = F.grid_sample(f[b:b + 1], grid[b:b + 1], mode="bilinear", padding_mode="border", align_corners=True)
            out.append(F.avg_pool2d(v, 2).reshape(CF, S, P, P).permute(1, 0, 2, 3))
        return torch.stack(out)

    fg = feat.clone().requires_grad_(True)

    def torch_both():
        fg.grad = None
        torch_forward(fg).backward(gp)

    def hip_fwd2():
        return RO.roi_align_forward(feat, rois, None, spec2)

    def hip_fwd0():
        return RO.roi_align_forward(feat, rois, None, spec0)

    def hip_bwd2():
        return RO.roi_align_backward(gp, rois, None, feat.shape, spec2, out=gf)

    def hip_bwd0():
        return RO.roi_align_backward(gp, rois, None, feat.shape, spec0, out=gf)

    lines = [f"RoIAlign at B={B} Cf={CF} map {HF}x{WF} S={S} bins {P}x{P} (pooled: {B * S * CF * P * P * 4 / 1e9:.2f} GB)"]
    a, t = hip_fwd2(), torch_forward()
    lines.append(f"  forward, HIP against torch ops: max abs difference {float((a - t).abs().max()):.3e}")
    del a, t
    torch_both()
    hip_bwd2()
    lines.append(f"  backward, HIP against torch autograd: max abs difference {float((gf - fg.grad).abs().max()):.3e} "
                 f"(max abs value {float(fg.grad.abs().max()):.3e})")
    tc = tile_counts(np, rois_np)
    lines.append(f"  backward cull: a tile walks {tc.mean():.0f} of an image's {S} RoIs on average (min {tc.min()}, max {tc.max()}); "
                 f"without the cull every tile would walk all {S}")
    fns = dict(hip_fwd2=hip_fwd2, hip_fwd0=hip_fwd0, torch_fwd=lambda: torch_forward(), hip_bwd2=hip_bwd2, hip_bwd0=hip_bwd0,
               torch_both=torch_both)
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    best = {k: 1e9 for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            best[k] = min(best[k], timed(torch, fn, args.iters))
    out_bytes = B * S * CF * P * P * 4
    lines.append(f"  HIP forward, sampling_ratio 2   {best['hip_fwd2']:.3f} ms  ({out_bytes / best['hip_fwd2'] / 1e9:.2f} TB/s written, "
                 f"{100 * out_bytes / best['hip_fwd2'] / 1e9 / HBM_STORE_TBS:.0f}% of {HBM_STORE_TBS} TB/s)")
    lines.append(f"  HIP forward, adaptive grid      {best['hip_fwd0']:.3f} ms  ({out_bytes / best['hip_fwd0'] / 1e9:.2f} TB/s written)")
    lines.append(f"  torch forward (grid_sample)     {best['torch_fwd']:.3f} ms")
    lines.append(f"  HIP backward, sampling_ratio 2  {best['hip_bwd2']:.3f} ms")
    lines.append(f"  HIP backward, adaptive grid     {best['hip_bwd0']:.3f} ms")
    tb = best['torch_both'] - best['torch_fwd']
    lines.append(f"  torch forward + backward        {best['torch_both']:.3f} ms  (backward alone: about {tb:.3f} ms, atomic scatter; "
                 f"HIP backward / torch backward = {best['hip_bwd2'] / max(tb, 1e-9):.2f})")
    lines.append(f"  (device events, best of {args.rounds} rounds of {args.iters} calls; the HIP times include the Python binding)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

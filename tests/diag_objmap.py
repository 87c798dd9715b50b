"""Diagnostic (not collected by pytest): the object-map classifier (gsr_objmap) at a working size -- 1080 x 1920, K = 256, one
view and five -- against the torch expression it replaces on the same device: torch.argmax(Conv2d(16, K, 1)(map), 1) for the
ids, and F.cross_entropy of the same logits with its autograd backward for the loss form.  The ids and the loss are compared
first (printed, not asserted).  Times come from device events after a warm-up, the variants alternating.  A report, not an
acceptance criterion.

    python tests/diag_objmap.py [--iters 5] [--rounds 3] [--out profiles/objmap_times.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W, K = 1080, 1920, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from diag_roi_detector import timed
    from diff_gaussian_rasterization import objmap_ops as OM

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    conv = torch.nn.Conv2d(16, K, 1).to(dev).requires_grad_(False)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(K, 16, 1, 1, generator=g) * 0.25).to(dev))
        conv.bias.copy_((torch.randn(K, generator=g) * 0.1).to(dev))
    wt, bs = conv.weight.view(K, 16).contiguous(), conv.bias.contiguous()
    lines = [f"object-map classifier at {W}x{H}, K={K}: the map is {16 * H * W * 4 / 1e6:.1f} MB per view, the torch expression's logits "
             f"{K * H * W * 4 / 1e9:.2f} GB per view"]
    print(lines[0], flush=True)
    for B in args.batches:
        x = (torch.rand((B, 16, H, W), generator=g) * torch.rand((B, 1, H, W), generator=g)).to(dev)
        t = torch.randint(0, K, (B, H, W), generator=g).to(dev)
        t32 = t.to(torch.int32)

        def hip_ids():
            return OM.objmap_forward(x, wt, bs).ids

        def hip_all():
            return OM.objmap_forward(x, wt, bs, want_conf=True, want_stats=True)

        def hip_loss():
            return OM.objmap_forward(x, wt, bs, target=t32, want_grad=True)

        def torch_ids():
            with torch.no_grad():
                return torch.argmax(conv(x), dim=1)

        def torch_loss():
            a = x.detach().requires_grad_(True)
            loss = F.cross_entropy(conv(a), t, reduction="none").mean(dim=(1, 2))
            loss.sum().backward()
            return loss.detach(), a.grad

        ids, ref_ids = hip_ids(), torch_ids()
        out, (ref_loss, ref_grad) = hip_loss(), torch_loss()
        hip_all()
        torch.cuda.synchronize()
        differ = int((ids.long() != ref_ids).sum())
        lines.append(f"B={B}: ids that differ from torch's {differ} of {ids.numel()}; loss, largest difference "
                     f"{(out.terms[:, 0] - ref_loss).abs().max().item():.3e} of {ref_loss.abs().max().item():.3f}; gradient "
                     f"{(out.grad - ref_grad).abs().max().item():.3e} of {ref_grad.abs().max().item():.3e}; second call bit-equal "
                     f"{torch.equal(hip_ids(), ids)} / {torch.equal(hip_loss().grad, out.grad)}")
        del out, ref_loss, ref_grad, ref_ids
        fns = dict(hip_ids=hip_ids, torch_ids=torch_ids, hip_all=hip_all, hip_loss=hip_loss, torch_loss=torch_loss)
        best = {k: 1e9 for k in fns}
        for r in range(args.rounds):
            for k, fn in fns.items():
                best[k] = min(best[k], timed(torch, fn, args.iters))
            print(f"  B={B} round {r} done", flush=True)
        n = B * H * W
        lines.append(f"  ids only,         gsr_objmap (one launch)              {best['hip_ids']:.3f} ms   "
                     f"({17 * n * 4 / best['hip_ids'] / 1e6:.0f} GB/s of the 17 n words moved, {2 * 16 * K * n / best['hip_ids'] / 1e9:.1f} TFLOP/s of the logits)")
        lines.append(f"  ids only,         torch: Conv2d + argmax               {best['torch_ids']:.3f} ms   (fused / torch = {best['hip_ids'] / best['torch_ids']:.3f})")
        lines.append(f"  ids, conf, stats, gsr_objmap (three launches)          {best['hip_all']:.3f} ms")
        lines.append(f"  ids, loss, grad,  gsr_objmap (three launches)          {best['hip_loss']:.3f} ms")
        lines.append(f"  loss, grad,       torch: Conv2d + cross_entropy + backward  {best['torch_loss']:.3f} ms   "
                     f"(fused / torch = {best['hip_loss'] / best['torch_loss']:.3f})")
        del x, t, t32
        torch.cuda.empty_cache()
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

"""Diagnostic: the groups set-up's selection (gsplat_attack.groups.select_group) timed on S-nyc-1M and S-airport-4K, with
a synthetic object of class 117 in a box of each city (scenes.synthetic_grouping):
  classify  k_group_classify (C = 256), HIP events;
  hull      IQR filter + quickhull on the host, wall clock;
  inside    k_points_in_hull over all P (fused OR with the mask), HIP events;
  total     the whole select_group call, wall clock with a device synchronise;
and, if scipy is present, the reference's formulation (torch Conv2d + softmax over [256, P], scipy Delaunay +
find_simplex over all P on the host, attack.py:306-315 / edit_object_removal.py:31-69) on S-nyc-1M.  Prints one line
per measurement.  python tests/diag_groups_select.py [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diff_gaussian_rasterization import groups as G  # noqa: E402
from gsplat_attack import groups as GA  # noqa: E402
from gsplat_attack.scenes import make_scene, synthetic_grouping  # noqa: E402

BOXES = {"nyc-1M": ((-6.0, -3.0, 1.0), (2.0, 5.0, 20.0)), "airport-4K": ((-30.0, -15.0, 1.0), (10.0, 25.0, 20.0))}


def _events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out, ts = None, []
    for _ in range(reps):
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return out, float(np.median(ts))


def _wall_ms(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    for key, (lo, hi) in BOXES.items():
        model, _, spec = make_scene(key, device=dev, n_views=1)
        xyz = model._xyz.detach()
        lo_t, hi_t = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
        rows = ((xyz >= lo_t) & (xyz <= hi_t)).all(dim=1)
        sd = synthetic_grouping(model, rows, 117)
        w, b = GA.load_classifier(sd)
        wd, bd = w.to(dev), b.to(dev)
        P = int(xyz.shape[0])
        (mask, _), t_cls = _events_ms(lambda: G.group_classify(model._objects_dc, wd, bd, [117], 0.5), reps)
        (hull, kept), t_hull = _wall_ms(lambda: GA._hull_of(xyz, mask, True, 1.0), reps)
        _, t_in = _events_ms(lambda: G.points_in_hull(xyz, hull, mask_in=mask), reps)
        (m3, info), t_all = _wall_ms(lambda: GA.select_group(model, (wd, bd), [117]), reps)
        print(f"[{spec.name}] P {P}: classify (C=256) {t_cls:.3f} ms, host hull {t_hull:.1f} ms ({kept} points, "
              f"{len(hull.planes)} facets), inside {t_in:.3f} ms, select_group {t_all:.1f} ms; {info}", flush=True)
        if key == "nyc-1M":
            try:
                from scipy.spatial import Delaunay
            except ImportError:
                print("[reference formulation] scipy missing: not timed")
                continue
            conv = torch.nn.Conv2d(16, 256, kernel_size=1).to(dev)
            conv.load_state_dict(sd)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)

            def ref_classify():
                with torch.no_grad():
                    prob = torch.softmax(conv(model._objects_dc.permute(2, 0, 1)), dim=0)
                    return (prob[torch.tensor([117], device=dev), :, :] > 0.5).any(dim=0).squeeze()
            rmask, t_rc = _wall_ms(ref_classify, reps)
            peak = (torch.cuda.max_memory_allocated(dev) - base) / 2**20
            if not torch.equal(rmask, mask):
                print(f"[reference formulation] classifier masks differ on {int((rmask != mask).sum())} Gaussians")

            def ref_hull():
                pts = xyz[rmask].cpu().numpy()
                filt = GA._iqr_filter(pts, 1.0)
                return Delaunay(filt).find_simplex(xyz.cpu().numpy()) >= 0
            inside, t_rh = _wall_ms(ref_hull, 1)
            agree = float(np.mean((inside | mask.cpu().numpy()) == m3.cpu().numpy()))
            print(f"[reference formulation, {spec.name}] conv + softmax {t_rc:.1f} ms (peak extra {peak:.0f} MB), "
                  f"Delaunay + find_simplex over all P {t_rh:.0f} ms; verdicts agree on {agree * 100:.4f} %", flush=True)


if __name__ == "__main__":
    main()

"""Diagnostic (not collected by pytest): the k-nearest-neighbour query at a working size, R = 1 000 000 references of the city
scene, in one run on one device:

  (a) gsr_knn_dist2 (distCUDA2): the unchanged 3-NN kernel of the same algorithm -- the yardstick for (b)
  (b) the self-query with k = 3 and exclusion (gsr_knn_query)
  (c) the k = 5 query of 50 000 points plus the gather-mean of the seven attribute tensors: the device side of inpaint_setup
  (d) the torch expression for (c) on the same device: chunked cdist + topk + index + mean

(b) is expected within 2x of (a): it also writes indices, keeps double slots and uses strict double arithmetic.  That margin
was a guess when it was written; the file says what was measured, with the query kernel's registers and occupancy.  Results
are compared first (printed, not asserted).  Times are device events after a warm-up, the variants alternating.  A report,
not an acceptance criterion.

    python tests/diag_knnq.py [--iters 3] [--rounds 3] [--out profiles/knnq_times.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

R, Q = 1_000_000, 50_000
RESOURCES = "k_knnq_query<3>: 85 VGPR, 5 waves/SIMD; <5>: 95 VGPR, 5 waves/SIMD; k_knn_search: 36 VGPR, 8 waves/SIMD; no scratch, no LDS"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from diag_roi_detector import timed
    from diff_gaussian_rasterization import knn_ops
    from gsplat_attack.scenes import city
    from simple_knn._C import distCUDA2

    dev = torch.device("cuda:0")
    a = city(R + Q, 7, 20.0, 60)
    order = ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity", "objects_dc")
    rest = [a[n][:R].float().contiguous().to(dev) for n in order]
    ref, qry = rest[0], a["xyz"][R:].float().contiguous().to(dev)
    del a

    def dist2():
        return distCUDA2(ref)

    def self3():
        return knn_ops.knn_query(ref)

    def inpaint():
        idx, _ = knn_ops.knn_query(ref, qry, k=5)
        return idx, knn_ops.gather_mean(idx, rest)

    def torch_inpaint(chunk=512):                       # [512, R] float32 distances: 2 GB at a time
        idx = torch.empty((Q, 5), dtype=torch.long, device=dev)
        for s in range(0, Q, chunk):
            idx[s:s + chunk] = torch.topk(torch.cdist(qry[s:s + chunk], ref), 5, dim=1, largest=False).indices
        return idx, [t[idx].mean(dim=1) for t in rest]

    d_a = dist2()
    i_b, d_b = self3()
    i_c, m_c = inpaint()
    i_d, m_d = torch_inpaint()
    torch.cuda.synchronize()
    mean_b = ((d_b[:, 0] + d_b[:, 1]) + d_b[:, 2]) / 3.0
    rel = ((mean_b - d_a).abs() / d_a.clamp_min(1e-30)).max().item()
    same = int((i_c.long().sort(dim=1).values == i_d.sort(dim=1).values).all(dim=1).sum())
    worst = max((x.reshape(Q, -1) - y.reshape(Q, -1)).abs().max().item() for x, y in zip(m_c, m_d))
    lines = [f"k-nearest-neighbour query, R = {R} references (city scene), one device",
             f"results: (b) mean of three d2 vs (a), largest relative difference {rel:.2e}; (c) vs (d): {same} of {Q} neighbour sets equal "
             f"(float32 cdist decides near-ties otherwise), largest difference of a mean {worst:.3e}"]
    fns = dict(a=dist2, b=self3, c=inpaint, d=torch_inpaint)
    best = {k: 1e9 for k in fns}
    for r in range(args.rounds):
        for k, fn in fns.items():
            best[k] = min(best[k], timed(torch, fn, args.iters if k != "d" else 1))
        print(f"  round {r} done", flush=True)
    lines += [f"  (a) gsr_knn_dist2, P = R                                        {best['a']:.3f} ms",
              f"  (b) gsr_knn_query self-query, k = 3, exclusion                  {best['b']:.3f} ms   (b / a = {best['b'] / best['a']:.2f}; expected <= 2)",
              f"  (c) gsr_knn_query k = 5, Q = {Q} + gsr_knn_gather_mean x 7   {best['c']:.3f} ms",
              f"  (d) torch: chunked cdist + topk + index + mean                  {best['d']:.3f} ms   (c / d = {best['c'] / best['d']:.4f})",
              f"  {RESOURCES}",
              f"  (device events, best of {args.rounds} rounds of {args.iters} calls, (d) one call per round; the times include the Python "
              "binding, the output allocations and, in (a) - (c), the one wait for the bounding box)"]
    if best["b"] > 2.0 * best["a"]:
        lines.append("  (b) is MORE than 2x (a): the double slots cost registers (85 VGPR against 36: 5 waves per SIMD against 8) and the "
                     "strict double arithmetic costs issue slots; gsr_knn_dist2 was not tuned to narrow this")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

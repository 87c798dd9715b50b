"""simple_knn._C -- the reference's second native import (``from simple_knn._C import distCUDA2``, reference
scene/gaussian_model.py:17; called at :144 in create_from_pcd to seed the initial scales).

On a HIP device it calls ``gsr_knn_dist2`` of libgsraster.so (uniform-grid exact 3-NN, csrc/gsr_knn.hip.h).  CPU tensors
-- which the reference never passes, its name says so -- get a chunked torch.cdist evaluation of the same definition,
so that a GaussianModel-style container can be exercised in CPU-only unit tests; that branch is not on the raster path.
With fewer than 4 points both branches follow the kernel's contract (csrc/gsr_knn.h): a missing neighbour counts as FLT_MAX,
summed and divided in float32 -- +inf for P <= 2, FLT_MAX / 3 for P = 3 -- so create_from_pcd gives the same scales on either.
"""
import torch


def _dist2_torch(pts: torch.Tensor) -> torch.Tensor:
    P = pts.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    k = min(4, P)
    chunk = max(1, min(P, (64 << 20) // max(4 * P, 1)))
    for s in range(0, P, chunk):
        d2 = torch.cdist(pts[s:s + chunk], pts).square_()
        near = torch.topk(d2, k, dim=1, largest=False).values[:, 1:]
        if k < 4:   # the kernel's contract (csrc/gsr_knn.h): a missing neighbour counts as FLT_MAX, summed and divided in float32
            near = torch.cat([near, near.new_full((near.shape[0], 4 - k), torch.finfo(torch.float32).max)], dim=1)
            out[s:s + chunk] = (near[:, 0] + near[:, 1] + near[:, 2]) / 3.0
        else:
            out[s:s + chunk] = near.mean(dim=1)
    return out


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    """Mean squared distance of every point to its 3 nearest neighbours, [P] float32."""
    pts = points.detach().float().contiguous()
    if not pts.is_cuda:
        return _dist2_torch(pts)
    import diff_gaussian_rasterization as D
    lib = D._load()
    P = int(pts.shape[0])
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    with torch.cuda.device(pts.device):
        rc = lib.gsr_knn_dist2(pts.data_ptr(), P, out.data_ptr(), D._stream(pts.device))
    if rc != 0:
        raise RuntimeError(D._err(lib))
    return out

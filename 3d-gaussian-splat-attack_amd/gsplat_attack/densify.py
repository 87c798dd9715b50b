"""Adaptive density control behind GaussianModel.add_densification_stats / densify_and_prune / prune_points (reference
``scene/gaussian_model.py:591-712``, schedule ``arguments/__init__.py:82-88`` and the densification block of the original 3D Gaussian Splatting training loop, which the reference itself does not ship).

On a HIP device the work is diff_gaussian_rasterization.densify_ops: one launch for the statistics, a classify + scan with ONE
read-back, one launch that moves every tensor, its Adam moments, the row mask and origin / kind.  Host tensors take the
tensor-op branch below, the same contract (csrc/gsr_densify.h) and what the CPU tests hold; on a device a library without
the entry points is an error, never a fall-back.

The contract in short (the header has it in full): per original row, g = accum / denom (NaN -> 0), hot = g >= max_grad,
smax = the largest RAW scale, o = the RAW opacity; thresholds in the log domain, formed in double and rounded once to float32:
t_dense = log(percent_dense extent), t_world = log(0.1 extent), t_opac = logit(min_opacity), c = log(0.8 N).
  split = hot and smax > t_dense;  pruned(s) = o < t_opac or (max_screen_size truthy and s > t_world)
  keep  = not split and not pruned(smax) [and not max_radii2D > max_screen_size with screen_prune]
  clone = hot and smax <= t_dense and not pruned(smax);  children = split and not pruned(smax - c)
Output rows: kept originals in row order, clones in parent order, children j-major.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

MAX_N = 8
KIND_KEEP, KIND_CLONE, KIND_CHILD = 0, 1, 2


@dataclass
class DensifyParams:
    """The reference's defaults (arguments/__init__.py:82-88) and the constants of its training loop."""
    densify_from_iter: int = 500
    densify_until_iter: int = 15000
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    densify_grad_threshold: float = 0.0002
    min_opacity: float = 0.005               # the original loop: densify_and_prune(threshold, 0.005, extent, size_threshold)
    size_threshold: float = 20.0             # ... size_threshold = 20 if iteration > opacity_reset_interval else None
    sh_degree_interval: int = 1000           # the original loop: oneupSHdegree every 1000 iterations
    extent: Optional[float] = None           # the scene's camera extent; None: model.spatial_lr_scale
    white_background: bool = False           # the original loop also resets the opacity at densify_from_iter on a white background
    N: int = 2
    seed: Optional[int] = None               # None: the model's counter
    screen_prune: bool = False

    def actions(self, iteration: int) -> Tuple[bool, bool, bool, Optional[float]]:
        """(raise the SH degree before the step, densify, reset the opacity, max_screen_size) at 1-based `iteration`,
        as the original training loop orders them: the degree at the top of the loop, the other two after the backward."""
        sh_up = iteration % self.sh_degree_interval == 0
        dens = reset = False
        size = None
        if iteration < self.densify_until_iter:
            if iteration > self.densify_from_iter and iteration % self.densification_interval == 0:
                dens = True
                size = self.size_threshold if iteration > self.opacity_reset_interval else None
            if iteration % self.opacity_reset_interval == 0 or (self.white_background and iteration == self.densify_from_iter):
                reset = True
        return sh_up, dens, reset, size


def thresholds(max_grad: float, min_opacity: float, extent: float, percent_dense: float, N: int, max_screen_size=None,
               screen_prune: bool = False) -> Dict[str, float]:
    """dens_thresholds of csrc/gsr_densify.h in Python floats: double arithmetic, rounded once to float32.  Raises a
    ValueError that names the argument whose threshold is not finite."""
    if not 1 <= int(N) <= MAX_N:
        raise ValueError(f"densify: N={N} (1..{MAX_N} children)")
    if screen_prune and not max_screen_size:
        raise ValueError("densify: screen_prune needs max_screen_size and max_radii")

    def f32(v):
        with np.errstate(over="ignore"):
            return float(np.float32(v))

    def log(v):
        return math.log(v) if v > 0 and math.isfinite(v) else float("nan")
    out = dict(max_grad=f32(max_grad), t_dense=f32(log(percent_dense * extent)), t_world=f32(log(0.1 * extent)),
               t_opac=f32(log(min_opacity / (1.0 - min_opacity)) if 0 < min_opacity < 1 else float("nan")), c=f32(math.log(0.8 * N)))
    out["max_screen"] = f32(max_screen_size or 0.0)
    if not math.isfinite(out["max_screen"]):
        raise ValueError(f"densify: max_screen_size={max_screen_size} is not a finite float32")
    if not math.isfinite(out["max_grad"]):
        raise ValueError(f"densify: max_grad={max_grad} is not a finite float32")
    if not (math.isfinite(out["t_dense"]) and math.isfinite(out["t_world"])):
        raise ValueError(f"densify: extent={extent} with percent_dense={percent_dense}: log(percent_dense extent) or log(0.1 extent) is not finite")
    if not math.isfinite(out["t_opac"]):
        raise ValueError(f"densify: min_opacity={min_opacity}: logit(min_opacity) is not finite (0 < min_opacity < 1)")
    return out


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def keyed_normals(seed: int, rows: np.ndarray, N: int) -> np.ndarray:
    """dens_normal of csrc/gsr_densify.h for the given rows: float32 [len(rows), N, 3], a function of (seed, row, child, axis)
    only.  The uniforms, the sine and the cosine are the header's operations; the logarithm is numpy's float32 one."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 1, 1)
    m = np.uint64(0xFFFFFFFF)
    base = _mix32((np.uint64(int(seed) & 0xFFFFFFFF) ^ ((rows * np.uint64(0x9E3779B9)) & m)) & m)
    child = np.arange(N, dtype=np.uint64).reshape(1, N, 1)
    pair = np.array([0, 0, 1], np.uint64).reshape(1, 1, 3)

    def uniform(which):
        k = _mix32((base + ((child << np.uint64(2)) | (pair << np.uint64(1)) | np.uint64(which))) & m)
        return ((k >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
    u1, u2 = uniform(0), uniform(1)
    f = np.float32
    rad = np.sqrt(f(-2.0) * np.log(u1))
    # dens_sincos_turn: every operation in float32, in the header's order
    t = f(4.0) * u2
    kf = np.floor(t + f(0.5))
    p = (t - kf) * f(1.5707963267948966)
    p2 = p * p
    sp = p * (f(1) + p2 * (f(-1.6666667e-1) + p2 * (f(8.3333333e-3) + p2 * (f(-1.9841270e-4) + p2 * f(2.7557319e-6)))))
    cp = f(1) + p2 * (f(-0.5) + p2 * (f(4.1666667e-2) + p2 * (f(-1.3888889e-3) + p2 * (f(2.4801587e-5) + p2 * f(-2.7557319e-7)))))
    k = kf.astype(np.int64) & 3
    sn = np.choose(k, [sp, cp, -sp, -cp])
    cs = np.choose(k, [cp, -sp, -cp, sp])
    trig = np.stack([cs[..., 0], sn[..., 1], cs[..., 2]], axis=-1)
    return (rad * trig).astype(np.float32)


def build_rotation(r: torch.Tensor) -> torch.Tensor:
    """utils/general_utils.py:78-99 in its order of operations: normalise, then the nine entries."""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def classify(accum, denom, scaling, opacity, max_radii, thr: Dict[str, float], max_screen_size, screen_prune: bool):
    """-> (keep, clone, kids) bool [P]: dens_classify of csrc/gsr_densify.h through tensor ops"""
    g = accum.reshape(-1) / denom.reshape(-1)
    g[g.isnan()] = 0.0
    smax = scaling.max(dim=1).values if scaling.shape[0] else scaling.new_zeros(0)          # torch.max: a NaN wins
    o = opacity.reshape(-1)
    hot = g >= thr["max_grad"]
    split = hot & (smax > thr["t_dense"])
    world = bool(max_screen_size)

    def pruned(s):
        p = o < thr["t_opac"]
        return p | (s > thr["t_world"]) if world else p
    own = pruned(smax)
    keep = ~split & ~own
    if screen_prune:
        keep = keep & ~(max_radii.reshape(-1) > thr["max_screen"])
    clone = hot & (smax <= thr["t_dense"]) & ~own
    kids = split & ~pruned(smax - thr["c"])
    return keep, clone, kids


def move_host(tensors: Dict[str, torch.Tensor], moments: Dict[str, Optional[Tuple[torch.Tensor, torch.Tensor]]], keep, clone, kids,
              N: int, c: float, normals: torch.Tensor):
    """The move of gsr_densify_apply through tensor ops.  tensors: name -> [P, ...] with xyz, scaling and rotation among them;
    normals [P, N, 3].  -> (new tensors, new moments, origin, kind)"""
    ki, ci, si = keep.nonzero().reshape(-1), clone.nonzero().reshape(-1), kids.nonzero().reshape(-1)
    out, mom = {}, {}
    for name, x in tensors.items():
        parts = [x[ki], x[ci]]
        if name == "xyz":
            R = build_rotation(tensors["rotation"][si])
            s = torch.exp(tensors["scaling"][si])
            for j in range(N):
                v = normals[si, j] * s
                parts.append(((R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]) + x[si])
        elif name == "scaling":
            parts += [x[si] - c] * N
        else:
            parts += [x[si]] * N
        out[name] = torch.cat(parts, dim=0).contiguous()
        mv = moments.get(name)
        if mv is not None:
            mom[name] = tuple(torch.cat([t[ki], torch.zeros((out[name].shape[0] - ki.numel(),) + tuple(t.shape[1:]), dtype=t.dtype)], dim=0)
                              for t in mv)
    origin = torch.cat([ki, ci] + [si] * N).to(torch.int32)
    kind = torch.cat([torch.full_like(ki, KIND_KEEP), torch.full_like(ci, KIND_CLONE)] +
                     [torch.full_like(si, KIND_CHILD + j) for j in range(N)]).to(torch.int32)
    return out, mom, origin, kind

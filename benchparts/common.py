"""Shared helpers of the benchmark.

Part of bench.py (the repo-root benchmark driver), split out in round 6: bench.py keeps the command line, the timed regions
of the headline metric and the assembly of the ONE JSON line; this module holds the source digest that ties PMC traffic figures to a build, logging, the algorithmic bytes per stage and
the output dump of --dump-outputs."""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def sources_digest() -> str:
    """SHA-256 over the library's sources (csrc/*, include/gsraster.h).  profiles/collect_r05.sh stores it next to the PMC
    counters it collects; a bench line quotes those counters as `roofline.traffic` only while the digest still matches --
    a kernel change silently keeping the old traffic figure was possible before."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    files.append(os.path.join(ROOT, "include", "gsraster.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


def log(msg: str) -> None:
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


DUMP_PIXELS = 131072      # pixels per view in an output dump (a fixed, seeded sample of the image)
DUMP_GAUSSIANS = 16384    # Gaussians per view in an output dump (a fixed, seeded sample)
DUMP_VIEWS = 8            # at most the last 8 views of the last launch chain
DUMP_CAP_BYTES = 64 << 20


def _sample(n: int, k: int, seed: int):
    """k sorted indices out of range(n), the same for every run with the same n (all of them when n <= k)."""
    import torch
    if n <= k:
        return torch.arange(n)
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values


def dump_outputs(out_dir: str, views: dict, per_gaussian: dict) -> list:
    """--dump-outputs: what the timed path handed its caller in the last step, as out_dir/<name>.npy (float32).
    `views`: name -> [B, C, H, W] images of the step's views (sampled at DUMP_PIXELS seeded pixels -> [B, C, K]);
    `per_gaussian`: name -> [B, P, ...] per-Gaussian arrays, or a list of B [P, ...] ones (radii, screen-space and attribute
    gradients, parameters; sampled at DUMP_GAUSSIANS seeded Gaussians -> [B, K, ...]).  At most the last DUMP_VIEWS views,
    at most 64 MB."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}
    for name, t in views.items():
        t = t[-DUMP_VIEWS:].detach()
        B, C = t.shape[0], t.shape[1]
        idx = _sample(t.shape[2] * t.shape[3], DUMP_PIXELS, 11).to(t.device)
        arrays[name] = t.reshape(B, C, -1).index_select(2, idx)
    for name, ts in per_gaussian.items():
        ts = list(ts)[-DUMP_VIEWS:]
        idx = _sample(ts[0].shape[0], DUMP_GAUSSIANS, 12).to(ts[0].device)
        arrays[name] = torch.stack([t.detach().index_select(0, idx) for t in ts])
    total = sum(a.numel() * 4 for a in arrays.values())
    assert total <= DUMP_CAP_BYTES, f"output dump of {total} bytes exceeds {DUMP_CAP_BYTES}"
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a.float().cpu().numpy())
    return sorted(arrays)


def stage_bytes(P: int, V: int, N: int, HW: int) -> dict:
    """Algorithmic bytes per launch of each stage (SURVEY.md section 8d derivation; objects off)."""
    return {
        "preprocess": 48 * P + 240 * V,          # K1: 44P in + 192V SH in, 48V geometry + 4P radii out
        "depth_sort": 0,                         # (the reference's single 64-bit pair sort is priced under tile_sort)
        "bin": 8 * P + 12 * N,                   # K2 scan + K3 emit
        "tile_sort": 24 * N,                     # K4 counted as ONE read + one write of the pairs (lower bound)
        "render_fwd": 40 * N + 20 * HW,          # K6
        "render_bwd": 20 * HW + 40 * N + 36 * V,  # K7
        "preprocess_bwd": 272 * V + 248 * P,     # K8+K9
    }

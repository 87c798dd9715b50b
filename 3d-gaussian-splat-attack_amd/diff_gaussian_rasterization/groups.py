"""ctypes bindings of the groups set-up's entry points (C ABI 603, include/gsraster.h):

  group_classify      per-Gaussian max selected softmax probability of a 1x1-conv classifier and its threshold mask
  convex_hull_planes  host quickhull (double) -> facet planes, bounding box, tau; no device needed
  points_in_hull      per-Gaussian hull inclusion, optionally OR-ed with a mask

No fallback: without libgsraster.so every call raises, and the two device calls need tensors on a HIP device.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import _err, _load, _stream

MAX_CLASSES = 1024
GSR_ERR_NOMEM = 3


_lib = _load              # (the entry points' signatures are declared in _signatures.py, applied by _load)


def _device_f32(t: torch.Tensor, device, name: str) -> torch.Tensor:
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise ValueError(f"{name} must be a tensor on a HIP device")
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def group_classify(objects: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, ids: Sequence[int],
                   thresh: float = 0.5):
    """objects [P,1,16] or [P,16], weight [C,16] (or [C,16,1,1]), bias [C] on one HIP device; ids: host ints.
    -> (mask [P] bool, psel [P] float32): psel = the largest softmax probability over `ids`, mask = psel > thresh."""
    if not (isinstance(objects, torch.Tensor) and objects.is_cuda):
        raise ValueError("group_classify: objects must be a tensor on a HIP device")
    dev = objects.device
    P = int(objects.shape[0])
    obj = _device_f32(objects, dev, "objects").reshape(P, -1)
    if obj.shape[1] != 16:
        raise ValueError(f"group_classify: objects have {obj.shape[1]} channels per Gaussian, expected 16")
    W = _device_f32(weight, dev, "weight")
    C = int(W.shape[0])
    W = W.reshape(C, -1)
    b = _device_f32(bias, dev, "bias").reshape(-1)
    if W.shape[1] != 16 or b.numel() != C:
        raise ValueError(f"group_classify: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} are not a Conv2d(16, C, 1)")
    ids_h = np.ascontiguousarray(np.asarray(list(ids), dtype=np.int64).astype(np.int32))
    psel = torch.empty(P, dtype=torch.float32, device=dev)
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    lib = _lib()
    with torch.cuda.device(dev):
        rc = lib.gsr_group_classify(obj.data_ptr() if P else None, P, W.data_ptr(), b.data_ptr(), C,
                                    ids_h.ctypes.data if ids_h.size else None, int(ids_h.size), float(thresh),
                                    psel.data_ptr() if P else None, mask.data_ptr() if P else None, _stream(dev))
    if rc != 0:
        raise ValueError(_err(lib)) if rc == 1 else RuntimeError(_err(lib))
    return mask.bool(), psel


class Hull(NamedTuple):
    planes: np.ndarray       # [F,4] float64: (nx, ny, nz, c), unit outward normals
    bbox: np.ndarray         # [6] float64: min xyz, max xyz of the points
    tau: float               # 1e-9 * bounding-box diagonal
    degenerate: bool         # F == 0: fewer than 4 points, or all of them within tau of a point, a line or a plane


def convex_hull_planes(points) -> Hull:
    """Convex hull of points [M,3] (array-like, taken as float64) on the host (gsr_convex_hull_planes)."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    M = int(pts.shape[0])
    lib = _lib()
    bbox = np.zeros(6, dtype=np.float64)
    nf = ctypes.c_int64(0)
    cap = max(16, min(2 * M, 1 << 16))
    while True:
        planes = np.zeros((cap, 4), dtype=np.float64)
        rc = lib.gsr_convex_hull_planes(pts.ctypes.data if M else None, M, planes.ctypes.data, cap, ctypes.byref(nf),
                                        bbox.ctypes.data)
        if rc == GSR_ERR_NOMEM and nf.value > cap:
            cap = int(nf.value)
            continue
        if rc != 0:
            raise (ValueError if rc == 1 else RuntimeError)(_err(lib))
        break
    F = int(nf.value)
    ext = bbox[3:] - bbox[:3]
    tau = 1e-9 * float(np.sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]))
    return Hull(planes[:F].copy(), bbox, tau, F == 0)


def points_in_hull(xyz: torch.Tensor, hull: Hull, mask_in: torch.Tensor = None) -> torch.Tensor:
    """xyz [P,3] on a HIP device -> [P] bool: inside `hull` (gsr_points_in_hull), OR-ed with mask_in when given."""
    if not (isinstance(xyz, torch.Tensor) and xyz.is_cuda):
        raise ValueError("points_in_hull: xyz must be a tensor on a HIP device")
    dev = xyz.device
    P = int(xyz.shape[0])
    pts = _device_f32(xyz, dev, "xyz").reshape(P, 3)
    F = int(hull.planes.shape[0])
    planes = torch.from_numpy(np.ascontiguousarray(hull.planes, dtype=np.float64).reshape(-1)).to(dev) if F else None
    bbox = torch.from_numpy(np.ascontiguousarray(hull.bbox, dtype=np.float64)).to(dev)
    m = None
    if mask_in is not None:
        m = mask_in.detach().reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
        if m.numel() != P:
            raise ValueError(f"points_in_hull: mask_in has {m.numel()} entries for {P} points")
    out = torch.empty(P, dtype=torch.uint8, device=dev)
    lib = _lib()
    with torch.cuda.device(dev):
        rc = lib.gsr_points_in_hull(pts.data_ptr() if P else None, P, planes.data_ptr() if F else None, F, bbox.data_ptr(),
                                    float(hull.tau), m.data_ptr() if (m is not None and P) else None,
                                    out.data_ptr() if P else None, _stream(dev))
    if rc != 0:
        raise (ValueError if rc == 1 else RuntimeError)(_err(lib))
    return out.bool()

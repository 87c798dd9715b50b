"""Exact k-nearest-neighbour queries with indices and the gather-mean over them (gsr_knn_query, gsr_knn_gather_mean of
include/gsraster.h; kernels csrc/gsr_knnq.hip.h, the contract csrc/gsr_knnq.h):

  available()    does the loaded library export the two entry points
  knn_query      the k nearest references of every query under the total order (d2 ascending, index ascending)
  gather_mean    per query the float32 rank-order mean of the neighbours' rows of any number of tensors

Tensors on a HIP device go to the kernels; a missing entry point is an error there, never a fall-back.  CPU tensors get a
chunked torch evaluation of the SAME definition -- float64 distances from coordinate differences, a stable sort by
(d2, index), a sequential float32 mean -- so that GaussianModel.inpaint_setup can be exercised in CPU-only unit tests, the
arrangement simple_knn/_C.py has for distCUDA2.  That branch is not on the device path.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from . import _err, _load, _stream

MAX_K = 8                     # KNNQ_MAX_K
MAX_TENSORS = 8               # per gsr_knn_gather_mean call
MAX_COLS = 128                # per tensor and per call
EXCLUDE_SAME_INDEX = 1        # GSR_KNNQ_EXCLUDE_SAME_INDEX


def available() -> bool:
    """True iff the library is there and exports gsr_knn_query and gsr_knn_gather_mean."""
    try:
        lib = _load()
    except (RuntimeError, OSError):
        return False
    return hasattr(lib, "gsr_knn_query") and hasattr(lib, "gsr_knn_gather_mean")


def _lib():
    lib = _load()
    if not (hasattr(lib, "gsr_knn_query") and hasattr(lib, "gsr_knn_gather_mean")):
        raise RuntimeError("knn_ops: the loaded libgsraster.so does not export gsr_knn_query / gsr_knn_gather_mean; rebuild it")
    return lib


def _raise(lib, rc):
    raise (ValueError if rc == 1 else RuntimeError)(_err(lib))


# ---- CPU: the same definition in torch -----------------------------------------------------------------------------------
def _query_torch(ref: torch.Tensor, qry: torch.Tensor, k: int, exclude: bool):
    R, Q = ref.shape[0], qry.shape[0]
    idx = torch.full((Q, k), -1, dtype=torch.int32)
    d2o = torch.full((Q, k), float("inf"), dtype=torch.float32)
    if R == 0 or Q == 0:
        return idx, d2o
    r64, q64 = ref.double(), qry.double()
    kk = min(k, R)
    chunk = max(1, (4 << 20) // R)
    for s in range(0, Q, chunk):
        q = q64[s:s + chunk]
        dx = r64[None, :, 0] - q[:, None, 0]
        dy = r64[None, :, 1] - q[:, None, 1]
        dz = r64[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[~torch.isfinite(d2)] = float("inf")                   # NaN and +inf distances are not neighbours
        if exclude:
            rows = torch.arange(q.shape[0])
            d2[rows, rows + s] = float("inf")
        val, order = torch.sort(d2, dim=1, stable=True)          # stable: equal distances in index order
        val, order = val[:, :kk], order[:, :kk]
        present = torch.isfinite(val)
        idx[s:s + chunk, :kk] = torch.where(present, order, torch.full_like(order, -1)).to(torch.int32)
        d2o[s:s + chunk, :kk] = val.to(torch.float32)            # (an absent slot is +inf already)
    return idx, d2o


def _gather_mean_torch(idx: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    R = t.shape[0]
    Q, k = idx.shape
    flat = t.reshape(R, int(torch.Size(t.shape[1:]).numel())).float()
    acc = torch.zeros(Q, flat.shape[1], dtype=torch.float32)
    m = torch.zeros(Q, dtype=torch.int64)
    for r in range(k):
        id_r = idx[:, r].long()
        ok = (id_r >= 0) & (id_r < R)
        rows = flat[id_r.clamp(0, max(R - 1, 0))] if R else torch.zeros_like(acc)
        first = ok & (m == 0)
        acc = torch.where(first[:, None], rows, torch.where(ok[:, None], acc + rows, acc))
        m = m + ok.long()
    out = torch.where((m > 0)[:, None], acc / m.clamp(min=1).to(torch.float32)[:, None], torch.zeros_like(acc))
    return out.reshape((Q,) + tuple(t.shape[1:]))


# ---- public -----------------------------------------------------------------------------------------------------------------
def knn_query(ref: torch.Tensor, qry: Optional[torch.Tensor] = None, k: int = 3,
              exclude_self: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ref [R,3], qry [Q,3] (None: the self-query, qry = ref with query i never taking reference i)
    -> (idx [Q,k] int32, d2 [Q,k] float32): the k nearest references of every query, nearest first, ties to the lower
    index; d2 = (dx*dx + dy*dy) + dz*dz in float64 rounded once to float32.  Missing neighbours (fewer than k references, the
    excluded one, non-finite points) are -1 / +inf.  exclude_self=True needs Q == R."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn_query: k={k} (1..{MAX_K})")
    if exclude_self is None:
        exclude_self = qry is None
    ref_t = ref.detach().to(torch.float32).reshape(-1, 3).contiguous()
    qry_t = ref_t if qry is None else qry.detach().to(device=ref_t.device, dtype=torch.float32).reshape(-1, 3).contiguous()
    R, Q = int(ref_t.shape[0]), int(qry_t.shape[0])
    if exclude_self and Q != R:
        raise ValueError(f"knn_query: exclude_self is the self-query, Q={Q} must equal R={R}")
    if not ref_t.is_cuda:
        return _query_torch(ref_t, qry_t, k, bool(exclude_self))
    lib = _lib()
    dev = ref_t.device
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((Q, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gsr_knn_query(ref_t.data_ptr() if R else None, R, qry_t.data_ptr() if Q else None, Q, k,
                               EXCLUDE_SAME_INDEX if exclude_self else 0, idx.data_ptr() if Q else None,
                               d2.data_ptr() if Q else None, _stream(dev))
    if rc != 0:
        _raise(lib, rc)
    return idx, d2


def gather_mean(idx: torch.Tensor, tensors: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """idx [Q,k] int32 (knn_query's), tensors: each [R, ...] float32 on idx's device -> for each a [Q, ...] tensor, element
    by element (((v0 + v1) + v2) ...) / m in float32 over the m present neighbours in rank order, 0 where there is none.
    Trailing dimensions are flattened into columns (at most 128 per tensor).  An index outside 0..R-1 counts as missing."""
    tensors = list(tensors)
    if idx.dim() != 2 or not 1 <= idx.shape[1] <= MAX_K:
        raise ValueError(f"gather_mean: idx must be [Q,k] with k in 1..{MAX_K}, got {tuple(idx.shape)}")
    if not tensors:
        return []
    R = int(tensors[0].shape[0])
    for t in tensors:
        if t.dim() < 1 or int(t.shape[0]) != R:
            raise ValueError("gather_mean: the tensors must share their first dimension")
        if t.device != idx.device:
            raise ValueError("gather_mean: idx and the tensors must be on one device")
    Q, k = int(idx.shape[0]), int(idx.shape[1])
    idx_t = idx.detach().to(torch.int32).contiguous()
    if not idx_t.is_cuda:
        return [_gather_mean_torch(idx_t, t.detach()) for t in tensors]
    lib = _lib()
    dev = idx_t.device
    cols = [int(torch.Size(t.shape[1:]).numel()) for t in tensors]
    srcs = [t.detach().to(torch.float32).reshape(R, c).contiguous() for t, c in zip(tensors, cols)]
    for c in cols:
        if not 1 <= c <= MAX_COLS:
            raise ValueError(f"gather_mean: {c} columns in one tensor (1..{MAX_COLS})")
    outs = [torch.empty((Q, c), dtype=torch.float32, device=dev) for c in cols]
    s = 0
    with torch.cuda.device(dev):
        while s < len(srcs):                                   # calls of at most 8 tensors and 128 columns
            e, total = s, 0
            while e < len(srcs) and e - s < MAX_TENSORS and total + cols[e] <= MAX_COLS:
                total += cols[e]
                e += 1
            n = e - s
            src_a = (ctypes.c_void_p * n)(*[srcs[i].data_ptr() if R else None for i in range(s, e)])
            dst_a = (ctypes.c_void_p * n)(*[outs[i].data_ptr() if Q else None for i in range(s, e)])
            col_a = (ctypes.c_int32 * n)(*cols[s:e])
            rc = lib.gsr_knn_gather_mean(idx_t.data_ptr() if Q else None, Q, k, R, n, src_a, col_a, dst_a, _stream(dev))
            if rc != 0:
                _raise(lib, rc)
            s = e
    return [o.reshape((Q,) + tuple(t.shape[1:])) for o, t in zip(outs, tensors)]

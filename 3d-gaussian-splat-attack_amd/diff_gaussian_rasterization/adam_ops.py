"""The fused Adam step (gsr_adam_step_multi of include/gsraster.h; kernel csrc/gsr_adam.hip.h, the contract csrc/gsr_adam.h):

  available()    does the loaded library export the entry point
  adam_step_     one step of up to 8 tensors of one model in ONE launch, in place, with an optional row mask / row range

Only contiguous float32 device tensors of [rows, <= 48 columns] are taken; anything else returns False with nothing
touched, and the caller (gsplat_attack.optim.GaussianAdam) runs the same arithmetic through tensor ops.  A missing entry
point on a device is an error, never a fall-back.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch

from ._ops_common import _load, call

MAX_TENSORS = 8               # ADAM_MAX_TENSORS
MAX_COLS = 48                 # ADAM_MAX_COLS


def available() -> bool:
    """True iff the library is there and exports gsr_adam_step_multi."""
    try:
        lib = _load()
    except (RuntimeError, OSError):
        return False
    return hasattr(lib, "gsr_adam_step_multi")


def _per_tensor(v, n: int):
    return [float(v)] * n if not isinstance(v, (list, tuple)) else [float(e) for e in v]


def adam_step_(items, step: int, lr, betas, eps, row_mask: Optional[torch.Tensor] = None,
               rows: Optional[Tuple[int, int]] = None) -> bool:
    """items: [(x, grad, m, v), ...], at most 8, each four tensors of one shape; step: the count of THIS step (>= 1);
    lr, eps: one float or one per tensor; betas: (beta1, beta2) or one pair per tensor; row_mask: None or a uint8 / bool
    device tensor [rows] (non-zero = the row moves); rows: None or (begin, end).  x, m and v are updated in place and
    every x has its version incremented.  True = the fused launch took the tensors; False = some tensor is not one it
    takes (a host tensor, another dtype or layout, more than 48 columns, more than 8 tensors): nothing was touched."""
    items = list(items)
    n = len(items)
    if not 1 <= n <= MAX_TENSORS:
        return False
    dev = items[0][0].device
    prepared = []
    for x, grad, m, v in items:
        x = x.detach()
        if not x.is_cuda or x.dim() < 1:
            return False
        for t in (grad, m, v):
            if t is None or t.device != dev or t.shape != x.shape or t.dtype != torch.float32 or not t.is_contiguous():
                return False
        if x.device != dev or x.dtype != torch.float32 or not x.is_contiguous():
            return False
        nrows = int(x.shape[0])
        cols = x.numel() // nrows if nrows else max(1, int(torch.Size(x.shape[1:]).numel()))
        if not 1 <= cols <= MAX_COLS:
            return False
        prepared.append((x, grad.detach(), m, v, nrows, cols))
    if row_mask is not None:
        if not row_mask.is_cuda or row_mask.device != dev or row_mask.dim() != 1 or not row_mask.is_contiguous() \
                or row_mask.dtype not in (torch.uint8, torch.bool):
            return False
        if any(p[4] != row_mask.shape[0] for p in prepared):
            raise ValueError(f"adam_step_: a row mask of {row_mask.shape[0]} entries for tensors of {[p[4] for p in prepared]} rows")
    if not hasattr(_load(), "gsr_adam_step_multi"):
        raise RuntimeError("adam_ops: the loaded libgsraster.so does not export gsr_adam_step_multi; rebuild it")
    lrs, epss = _per_tensor(lr, n), _per_tensor(eps, n)
    pairs = [tuple(betas)] * n if not isinstance(betas[0], (list, tuple)) else [tuple(b) for b in betas]
    begin, end = (0, -1) if rows is None else (int(rows[0]), int(rows[1]))
    ptrs = lambda k: (ctypes.c_void_p * n)(*[p[k].data_ptr() if p[4] else None for p in prepared])   # noqa: E731
    f32s = lambda vals: (ctypes.c_float * n)(*vals)   # noqa: E731
    call("gsr_adam_step_multi", dev, n, ptrs(0), ptrs(1), ptrs(2), ptrs(3), (ctypes.c_int64 * n)(*[p[4] for p in prepared]),
         (ctypes.c_int32 * n)(*[p[5] for p in prepared]), f32s(lrs), f32s([b[0] for b in pairs]), f32s([b[1] for b in pairs]),
         f32s(epss), int(step), None if row_mask is None else row_mask.data_ptr(), begin, end)
    # the kernel wrote through the raw pointers: tell autograd (a rasteriser forward that saved a parameter and has not run
    # its backward yet must see the change, diff_gaussian_rasterization checks the versions)
    for p in prepared:
        torch.autograd.graph.increment_version(p[0])
    return True

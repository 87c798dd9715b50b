"""Adaptive density control (gsr_densify_stats / gsr_densify_plan / gsr_densify_apply of include/gsraster.h; kernels
csrc/gsr_densify.hip.h, the contract csrc/gsr_densify.h):

  available()   does the loaded library export the entry points
  stats_        the densification statistics of one view or a batch of views, in place, one launch
  plan          classify the rows and scan the three counts: ONE read-back (the counts), so the outputs can be sized
  plan_prune    the same from a byte mask: a plain prune
  apply         move every tensor, its moments, the row mask and origin / kind to their new rows in ONE launch

Only contiguous float32 device tensors are taken.  A missing entry point on a device is an error, never a fall-back; host
tensors take gsplat_attack.gaussian_model's tensor-op branch of the same contract.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from ._ops_common import _load, _need_device, _raise, call, workspace

MAX_TENSORS = 8               # DENS_MAX_TENSORS
MAX_COLS = 48                 # DENS_MAX_COLS
MAX_N = 8                     # DENS_MAX_N
COPY, XYZ, SCALE = 0, 1, 2    # a tensor's role in the move
WORLD_PRUNE, SCREEN_PRUNE = 1, 2
_SYMBOLS = ("gsr_densify_stats", "gsr_densify_plan_bytes", "gsr_densify_plan", "gsr_densify_plan_prune", "gsr_densify_apply")


def available() -> bool:
    """True iff the library is there and exports the four entry points."""
    try:
        lib = _load()
    except (RuntimeError, OSError):
        return False
    return all(hasattr(lib, s) for s in _SYMBOLS)


def _lib():
    lib = _load()
    for s in _SYMBOLS:
        if not hasattr(lib, s):
            raise RuntimeError(f"densify_ops: the loaded libgsraster.so does not export {s}; rebuild it")
    return lib


def _f32c(t: torch.Tensor, fn: str, name: str) -> torch.Tensor:
    _need_device(t, fn, name)
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous float32 tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    return t


def stats_(grad: torch.Tensor, accum: torch.Tensor, denom: torch.Tensor, radii: Optional[torch.Tensor] = None,
           update_filter: Optional[torch.Tensor] = None, max_radii: Optional[torch.Tensor] = None) -> None:
    """grad [P,3] or [B,P,3] (the screen-space gradient, x and y read); accum, denom [P] or [P,1], updated in place; radii
    [P] / [B,P] integer (with update_filter None it is the filter: radii > 0); update_filter [P] / [B,P] bool or uint8;
    max_radii [P]: also folds max(max_radii, radii).  The views of a batch are taken in order: bit for bit B single calls."""
    fn = "densify_ops.stats_"
    grad = _f32c(grad, fn, "grad")
    accum, denom = _f32c(accum, fn, "accum"), _f32c(denom, fn, "denom")
    if grad.dim() == 2:
        grad = grad[None]
    B, P = int(grad.shape[0]), int(grad.shape[1])
    if grad.dim() != 3 or grad.shape[2] != 3 or accum.numel() != P or denom.numel() != P:
        raise ValueError(f"{fn}: grad {tuple(grad.shape)}, accum {tuple(accum.shape)}, denom {tuple(denom.shape)}")
    dev = grad.device
    if radii is not None:
        radii = radii.detach().to(device=dev, dtype=torch.int32).contiguous()
        if radii.numel() != B * P:
            raise ValueError(f"{fn}: radii {tuple(radii.shape)} for {B} views of {P} Gaussians")
    if update_filter is not None:
        f = update_filter.detach().to(dev)
        update_filter = (f if f.dtype in (torch.bool, torch.uint8) else f != 0).contiguous()
        if update_filter.numel() != B * P:
            raise ValueError(f"{fn}: filter {tuple(update_filter.shape)} for {B} views of {P} Gaussians")
    if max_radii is not None:
        max_radii = _f32c(max_radii, fn, "max_radii")
        if max_radii.numel() != P:
            raise ValueError(f"{fn}: max_radii {tuple(max_radii.shape)} for {P} Gaussians")
    _lib()
    call("gsr_densify_stats", dev, grad.data_ptr(), None if radii is None else radii.data_ptr(),
         None if update_filter is None else update_filter.data_ptr(), B, P, accum.data_ptr(), denom.data_ptr(),
         None if max_radii is None else max_radii.data_ptr())


@dataclass
class Plan:
    """What gsr_densify_plan leaves: the counts on the host and the codes and offsets in `ws` on the device."""
    P: int
    N: int
    n_keep: int
    n_clone: int
    n_split: int
    ws: Optional[torch.Tensor]
    device: torch.device

    @property
    def rows_out(self) -> int:
        return self.n_keep + self.n_clone + self.N * self.n_split


def plan(accum: torch.Tensor, denom: torch.Tensor, scaling: torch.Tensor, opacity: torch.Tensor, *, max_grad: float,
         min_opacity: float, extent: float, percent_dense: float, max_screen_size=None, N: int = 2, screen_prune: bool = False,
         max_radii: Optional[torch.Tensor] = None) -> Plan:
    """Classify the P rows (csrc/gsr_densify.h) and scan the three counts; waits for the stream once, for the counts.
    max_screen_size truthy: the world-size prune acts (the reference's live test); screen_prune: also max_radii > it."""
    fn = "densify_ops.plan"
    accum, denom = _f32c(accum, fn, "accum"), _f32c(denom, fn, "denom")
    scaling, opacity = _f32c(scaling, fn, "scaling"), _f32c(opacity, fn, "opacity")
    P = int(scaling.shape[0])
    if scaling.numel() != 3 * P or opacity.numel() != P or accum.numel() != P or denom.numel() != P:
        raise ValueError(f"{fn}: scaling {tuple(scaling.shape)}, opacity {tuple(opacity.shape)}, accum {tuple(accum.shape)}, denom {tuple(denom.shape)}")
    flags = (WORLD_PRUNE if max_screen_size else 0) | (SCREEN_PRUNE if screen_prune else 0)
    if screen_prune:
        if not max_screen_size or max_radii is None:
            raise ValueError(f"{fn}: screen_prune needs max_screen_size and max_radii")
        max_radii = _f32c(max_radii, fn, "max_radii")
        if max_radii.numel() != P:
            raise ValueError(f"{fn}: max_radii {tuple(max_radii.shape)} for {P} Gaussians")
    lib, dev = _lib(), scaling.device
    nbytes = ctypes.c_int64(0)
    rc = lib.gsr_densify_plan_bytes(P, ctypes.byref(nbytes))
    if rc != 0:
        _raise(lib, rc)
    ws = workspace(int(nbytes.value), dev)
    counts = (ctypes.c_int64 * 3)()
    call("gsr_densify_plan", dev, accum.data_ptr(), denom.data_ptr(), scaling.data_ptr(), opacity.data_ptr(),
         max_radii.data_ptr() if screen_prune else None, P, float(max_grad), float(min_opacity), float(extent), float(percent_dense),
         float(max_screen_size or 0.0), int(N), flags, ws.data_ptr(), ws.numel() * 8, counts)
    return Plan(P, int(N), int(counts[0]), int(counts[1]), int(counts[2]), ws, dev)


def plan_prune(prune_mask: torch.Tensor) -> Plan:
    """The plan of a plain prune: prune_mask bool / uint8 [P], non-zero = the row goes.  No clone, no split; one wait."""
    fn = "densify_ops.plan_prune"
    _need_device(prune_mask, fn, "prune_mask")
    m = prune_mask.detach().reshape(-1)
    m = (m if m.dtype in (torch.bool, torch.uint8) else m != 0).contiguous()
    P = int(m.numel())
    lib, dev = _lib(), m.device
    nbytes = ctypes.c_int64(0)
    rc = lib.gsr_densify_plan_bytes(P, ctypes.byref(nbytes))
    if rc != 0:
        _raise(lib, rc)
    ws = workspace(int(nbytes.value), dev)
    counts = (ctypes.c_int64 * 3)()
    call("gsr_densify_plan_prune", dev, m.data_ptr() if P else None, P, ws.data_ptr(), ws.numel() * 8, counts)
    return Plan(P, 1, int(counts[0]), 0, 0, ws, dev)


def apply(pl: Plan, items: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], int]], rotation: torch.Tensor, *,
          seed: int = 0, normals: Optional[torch.Tensor] = None, row_mask: Optional[torch.Tensor] = None, want_mask: bool = False,
          want_origin: bool = True, out=None):
    """items: [(tensor [P, ...], exp_avg or None, exp_avg_sq or None, role), ...]; rotation [P,4]: the raw quaternions the
    children's positions are built from; normals: None (keyed by seed) or [P,N,3] standard normals; row_mask: None or uint8 /
    bool [P].  -> (outs, mask_out, origin, kind): outs[i] = (tensor [P', ...], exp_avg, exp_avg_sq) all new; mask_out uint8
    [P'] or None (given when row_mask is, or want_mask); origin / kind int32 [P'] or None.  More than 8 tensors go in
    several launches over the same plan; a tensor with no columns comes back empty.  out: None, or what an earlier apply of the same
    plan, items and options returned: it is written again and returned, nothing is allocated."""
    fn = "densify_ops.apply"
    lib, dev, P, Pn = _lib(), pl.device, pl.P, pl.rows_out
    rotation = _f32c(rotation, fn, "rotation")
    if rotation.numel() != 4 * P:
        raise ValueError(f"{fn}: rotation {tuple(rotation.shape)} for {P} Gaussians")
    if normals is not None:
        normals = _f32c(normals, fn, "normals")
        if tuple(normals.shape) != (P, pl.N, 3):
            raise ValueError(f"{fn}: normals {tuple(normals.shape)}, expected {(P, pl.N, 3)}")
    mask_in = None
    if row_mask is not None:
        _need_device(row_mask, fn, "row_mask")
        mask_in = row_mask.detach()
        mask_in = (mask_in if mask_in.dtype in (torch.bool, torch.uint8) else mask_in != 0).reshape(-1).contiguous()
        if mask_in.numel() != P:
            raise ValueError(f"{fn}: a row mask of {mask_in.numel()} entries for {P} Gaussians")
    if out is not None:
        outs, mask_out, origin, kind = list(out[0]), out[1], out[2], out[3]
        if len(outs) != len(items) or any(o[0].shape[0] != Pn for o in outs):
            raise ValueError(f"{fn}: out does not belong to this plan and these items")
    else:
        mask_out = torch.empty(Pn, dtype=torch.uint8, device=dev) if (mask_in is not None or want_mask) else None
        origin = torch.empty(Pn, dtype=torch.int32, device=dev) if want_origin else None
        kind = torch.empty(Pn, dtype=torch.int32, device=dev) if want_origin else None
        outs: List[Optional[tuple]] = [None] * len(items)
    live = []
    for i, (x, m, v, role) in enumerate(items):
        x = _f32c(x, fn, f"tensor {i}")
        if x.dim() < 1 or int(x.shape[0]) != P:
            raise ValueError(f"{fn}: tensor {i} has shape {tuple(x.shape)}, the plan {P} rows")
        cols = int(torch.Size(x.shape[1:]).numel())
        if (m is None) != (v is None):
            raise ValueError(f"{fn}: tensor {i}: exp_avg and exp_avg_sq come together")
        if m is not None:
            m, v = _f32c(m, fn, f"exp_avg {i}"), _f32c(v, fn, f"exp_avg_sq {i}")
            if m.shape != x.shape or v.shape != x.shape:
                raise ValueError(f"{fn}: tensor {i}: moments of shape {tuple(m.shape)} / {tuple(v.shape)} for {tuple(x.shape)}")
        shape = (Pn,) + tuple(x.shape[1:])
        new = lambda: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        if out is None:
            outs[i] = (new(), None if m is None else new(), None if m is None else new())
        elif tuple(outs[i][0].shape) != shape or (outs[i][1] is None) != (m is None):
            raise ValueError(f"{fn}: out[{i}] does not belong to this plan and these items")
        if cols == 0:
            continue
        if cols > MAX_COLS:
            raise ValueError(f"{fn}: tensor {i} has {cols} columns (at most {MAX_COLS})")
        live.append((x, m, v, int(role), cols, outs[i]))
    # the XYZ tensor's children read the SCALE tensor: the two go in one launch
    live.sort(key=lambda e: e[3] == COPY)
    counts = (ctypes.c_int64 * 3)(pl.n_keep, pl.n_clone, pl.n_split)
    first = True
    for s in range(0, max(len(live), 1), MAX_TENSORS):
        part = live[s:s + MAX_TENSORS]
        n = len(part)
        arr = lambda vals: (ctypes.c_void_p * max(n, 1))(*[None if t is None else t.data_ptr() for t in vals])   # noqa: E731
        has_state = any(e[1] is not None for e in part)
        tables = [arr([e[1] for e in part]), arr([e[2] for e in part]), arr([e[5][1] for e in part]), arr([e[5][2] for e in part])] \
            if has_state else [None] * 4
        call("gsr_densify_apply", dev, None if pl.ws is None else pl.ws.data_ptr(), 0 if pl.ws is None else pl.ws.numel() * 8, P, counts, n,
             arr([e[0] for e in part]), arr([e[5][0] for e in part]), *tables, (ctypes.c_int32 * max(n, 1))(*[e[4] for e in part]),
             (ctypes.c_int32 * max(n, 1))(*[e[3] for e in part]), rotation.data_ptr(), pl.N, int(seed) & 0xFFFFFFFF,
             None if normals is None else normals.data_ptr(), None if (mask_in is None or not first) else mask_in.data_ptr(),
             None if (mask_out is None or not first) else mask_out.data_ptr(), None if (origin is None or not first) else origin.data_ptr(),
             None if (kind is None or not first) else kind.data_ptr())
        first = False
    return outs, mask_out, origin, kind

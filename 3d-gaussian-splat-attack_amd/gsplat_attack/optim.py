"""Fitting a model: the optimiser of the reference's three set-ups and the plain refit loop.

Counterpart of the reference's ``scene/gaussian_model.py:160-214,350-375,558-650`` (training_setup, finetune_setup, the tail
of inpaint_setup, update_learning_rate, _prune_optimizer / cat_tensors_to_optimizer / replace_tensor_to_optimizer),
``arguments/__init__.py`` (OptimizationParams) and ``utils/general_utils.py:29-61`` (get_expon_lr_func):

  OptimizationParams   the reference's learning rates
  get_expon_lr_func    the position schedule
  GaussianAdam         torch.optim.Adam(l, lr=0.0, eps=1e-15) over the model's seven named groups, as ONE fused launch per
                       step (diff_gaussian_rasterization.adam_ops.adam_step_: gsr_adam_step_multi), with an optional row
                       mask or row range: rows left out are neither read nor written
  refit                update_learning_rate, render, photometric_loss, backward, step, zero_grad; with densify= the original
                       densification schedule (gsplat_attack.densify)

The arithmetic of a step is csrc/gsr_adam.h's: m' = m + (1 - b1)(g - m); v' = b2 v + (1 - b2)(g g);
den = sqrt(v') / sqrt_bc2 + eps; x' = x - step_size (m' / den), every operation rounded once in float32, with
step_size = lr / (1 - b1^t) and sqrt_bc2 = sqrt(1 - b2^t) formed in double and rounded once.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn


@dataclass
class OptimizationParams:
    """The reference's defaults (arguments/__init__.py: OptimizationParams)."""
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30000
    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    percent_dense: float = 0.01


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """step -> learning rate: lr_init at step 0, lr_final at max_steps, log-linear between (clamped outside), eased in
    over lr_delay_steps by lr_delay_mult + (1 - lr_delay_mult) sin(pi / 2 * clip(step / lr_delay_steps, 0, 1)).  A negative
    step, or both rates zero, gives 0.  The arithmetic of expon_lr in csrc/gsr_adam.h, in Python floats."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        else:
            delay_rate = 1.0
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay_rate * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return helper


GROUP_ATTRS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
               ("scaling", "_scaling"), ("rotation", "_rotation"), ("obj_dc", "_objects_dc"))    # the reference's order


def reference_groups(opt: OptimizationParams, spatial_lr_scale: float = 1.0) -> List[dict]:
    """The seven (name, lr) of reference scene/gaussian_model.py:165-173."""
    lrs = dict(xyz=opt.position_lr_init * spatial_lr_scale, f_dc=opt.feature_lr, f_rest=opt.feature_lr / 20.0,
               opacity=opt.opacity_lr, scaling=opt.scaling_lr, rotation=opt.rotation_lr, obj_dc=opt.feature_lr)
    return [dict(name=n, lr=lrs[n]) for n, _ in GROUP_ATTRS]


def bias_corrections(lr: float, beta1: float, beta2: float, step: int) -> Tuple[float, float]:
    """(step_size, sqrt_bc2) as float32 values: adam_bias_corrections of csrc/gsr_adam.h on the float32 lr and betas."""
    lr, beta1, beta2 = float(np.float32(lr)), float(np.float32(beta1)), float(np.float32(beta2))
    return (float(np.float32(lr / (1.0 - math.pow(beta1, float(step))))),
            float(np.float32(math.sqrt(1.0 - math.pow(beta2, float(step))))))


_WARNED = set()


class GaussianAdam:
    """Adam over named tensors of a GaussianModel.  groups: dicts with `name` (one of xyz, f_dc, f_rest, opacity, scaling,
    rotation, obj_dc) and `lr`; row_mask: None or a bool / uint8 tensor [P] (non-zero = the row moves); rows: None or a row
    range (begin, end).  Both select rows for every group; rows left out keep their parameter and moments bit for bit."""

    def __init__(self, model, groups: Sequence[dict], eps: float = 1e-15, betas: Tuple[float, float] = (0.9, 0.999),
                 row_mask: Optional[torch.Tensor] = None, rows: Optional[Tuple[int, int]] = None):
        attrs = dict(GROUP_ATTRS)
        self.model = model
        self.eps, self.betas = float(eps), (float(betas[0]), float(betas[1]))
        self.param_groups: List[dict] = []
        for g in groups:
            if g["name"] not in attrs:
                raise ValueError(f"GaussianAdam: unknown group {g['name']!r}")
            self.param_groups.append(dict(name=g["name"], lr=float(g["lr"]), params=[getattr(model, attrs[g["name"]])]))
        self.state: Dict[str, dict] = {}
        self.step_count = 0
        P = int(model._xyz.shape[0])
        self.row_mask = None
        if row_mask is not None:
            row_mask = row_mask.detach().reshape(-1)
            if row_mask.numel() != P:
                raise ValueError(f"GaussianAdam: row mask of {row_mask.numel()} entries for {P} Gaussians")
            self.row_mask = (row_mask != 0).to(device=model._xyz.device, dtype=torch.uint8).contiguous()
        self.rows = None
        if rows is not None:
            b, e = int(rows[0]), int(rows[1])
            if not 0 <= b <= e <= P:
                raise ValueError(f"GaussianAdam: row range [{b}, {e}) of {P} rows")
            self.rows = (b, e)

    # ---- the step -----------------------------------------------------------------------------------------------------
    def _attr(self, name: str) -> str:
        return dict(GROUP_ATTRS)[name]

    def _active(self):
        """the groups that step: a parameter with a gradient (torch skips grad None; a frozen tensor has none)"""
        out = []
        for g in self.param_groups:
            p = g["params"][0]
            if p.grad is None or not p.requires_grad:
                continue
            st = self.state.get(g["name"])
            if st is None:
                st = self.state[g["name"]] = dict(exp_avg=torch.zeros_like(p, memory_format=torch.preserve_format),
                                                  exp_avg_sq=torch.zeros_like(p, memory_format=torch.preserve_format))
            out.append((g, p, st))
        return out

    @torch.no_grad()
    def step(self) -> None:
        active = self._active()
        if not active:
            return
        devices = {p.device for _, p, _ in active} | ({self.row_mask.device} if self.row_mask is not None else set())
        if len(devices) != 1:
            raise ValueError(f"GaussianAdam.step: the parameters and the row mask must live on one device, got {sorted(map(str, devices))}")
        self.step_count += 1
        t = self.step_count
        from diff_gaussian_rasterization import adam_ops
        if all(p.is_cuda for _, p, _ in active):
            for s in range(0, len(active), adam_ops.MAX_TENSORS):
                part = active[s:s + adam_ops.MAX_TENSORS]
                items = [(p, p.grad, st["exp_avg"], st["exp_avg_sq"]) for _, p, st in part]
                if not adam_ops.adam_step_(items, t, [g["lr"] for g, _, _ in part], self.betas, self.eps, self.row_mask, self.rows):
                    key = tuple((p.dtype, p.is_contiguous()) for _, p, _ in part)
                    if key not in _WARNED:
                        _WARNED.add(key)
                        warnings.warn("gsplat_attack.optim: gsr_adam_step_multi updates contiguous float32 [rows, <=48] tensors; "
                                      f"these ({[(str(p.dtype), p.is_contiguous(), tuple(p.shape)) for _, p, _ in part]}) take "
                                      "the tensor-op formulation instead", stacklevel=2)
                    for g, p, st in part:
                        self._tensor_step(p, p.grad, st, g["lr"], t)
            return
        for g, p, st in active:                     # host tensors: the formulation the CPU tests hold
            self._tensor_step(p, p.grad, st, g["lr"], t)

    def _live(self, P: int, dev) -> Optional[torch.Tensor]:
        if self.row_mask is None and self.rows is None:
            return None
        live = torch.ones(P, dtype=torch.bool, device=dev) if self.row_mask is None else self.row_mask.to(dev) != 0
        if self.rows is not None:
            inside = torch.zeros(P, dtype=torch.bool, device=dev)
            inside[self.rows[0]:self.rows[1]] = True
            live = live & inside
        return live

    def _tensor_step(self, p, grad, st, lr: float, t: int) -> None:
        """csrc/gsr_adam.h's sequence of single operations through tensor ops, on the live rows"""
        b1, b2 = float(np.float32(self.betas[0])), float(np.float32(self.betas[1]))
        eps = float(np.float32(self.eps))
        ss, sb = bias_corrections(lr, b1, b2, t)
        w1, w2 = float(np.float32(1.0 - b1)), float(np.float32(1.0 - b2))
        live = self._live(int(p.shape[0]), p.device)
        x, m, v = p.detach(), st["exp_avg"], st["exp_avg_sq"]
        g = grad.detach().to(x.dtype)
        if live is not None:
            x_, g, m_, v_ = x[live], g[live], m[live], v[live]
        else:
            x_, m_, v_ = x, m, v
        gm = g - m_
        m1 = m_ + gm * w1
        v1 = v_ * b2 + (g * g) * w2
        den = v1.sqrt() / sb + eps
        x1 = x_ - (m1 / den) * ss
        if live is not None:
            x[live], m[live], v[live] = x1, m1, v1
        else:
            x.copy_(x1)
            m.copy_(m1)
            v.copy_(v1)

    def zero_grad(self, set_to_none: bool = True) -> None:
        for g in self.param_groups:
            p = g["params"][0]
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    # ---- state ----------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        return dict(step=self.step_count, eps=self.eps, betas=self.betas, rows=self.rows,
                    row_mask=None if self.row_mask is None else self.row_mask.clone(),
                    param_groups=[dict(name=g["name"], lr=g["lr"]) for g in self.param_groups],
                    state={n: {k: t.clone() for k, t in st.items()} for n, st in self.state.items()})

    def load_state_dict(self, sd: dict) -> None:
        names = [g["name"] for g in self.param_groups]
        if [g["name"] for g in sd["param_groups"]] != names:
            raise ValueError("GaussianAdam.load_state_dict: the groups differ")
        by_name = {g["name"]: g for g in self.param_groups}
        for n, st in sd["state"].items():
            p = by_name[n]["params"][0]
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(st[k].shape) != tuple(p.shape):
                    raise ValueError(f"GaussianAdam.load_state_dict: {n}.{k} has shape {tuple(st[k].shape)}, the parameter {tuple(p.shape)}")
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g["lr"] = float(s["lr"])
        self.step_count, self.eps, self.betas = int(sd["step"]), float(sd["eps"]), tuple(sd["betas"])
        self.rows = None if sd["rows"] is None else (int(sd["rows"][0]), int(sd["rows"][1]))
        dev = self.model._xyz.device
        self.row_mask = None if sd["row_mask"] is None else sd["row_mask"].to(device=dev, dtype=torch.uint8).clone()
        self.state = {n: {k: st[k].to(device=by_name[n]["params"][0].device, dtype=by_name[n]["params"][0].dtype).clone()
                          for k in ("exp_avg", "exp_avg_sq")} for n, st in sd["state"].items()}

    # ---- state surgery (torch indexing; not a hot path) --------------------------------------------------------------------
    def _rewrap(self, g: dict, data: torch.Tensor) -> nn.Parameter:
        old = g["params"][0]
        new = nn.Parameter(data.contiguous(), requires_grad=old.requires_grad)
        g["params"][0] = new
        setattr(self.model, self._attr(g["name"]), new)
        return new

    def prune(self, keep_mask: torch.Tensor) -> Dict[str, nn.Parameter]:
        """Keep the rows keep_mask selects (reference _prune_optimizer / prune_points): parameters, moments and the row mask
        follow their rows; a row range shrinks to the kept rows inside it."""
        keep = keep_mask.detach().reshape(-1).bool()
        out = {}
        with torch.no_grad():
            for g in self.param_groups:
                p = g["params"][0]
                k = keep.to(p.device)
                st = self.state.get(g["name"])
                if st is not None:
                    st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][k].contiguous(), st["exp_avg_sq"][k].contiguous()
                out[g["name"]] = self._rewrap(g, p.detach()[k].clone())
        if self.row_mask is not None:
            self.row_mask = self.row_mask[keep.to(self.row_mask.device)].contiguous()
        if self.rows is not None:
            b = int(keep[:self.rows[0]].sum())
            self.rows = (b, b + int(keep[self.rows[0]:self.rows[1]].sum()))
        return out

    def append(self, tensors_dict: Dict[str, torch.Tensor]) -> Dict[str, nn.Parameter]:
        """Append rows to every group (reference cat_tensors_to_optimizer / densification_postfix): tensors_dict maps every
        group name to its new rows.  New rows have zero moments and move: a row mask is extended with ones, a row range
        that ends at the last row is extended, any other range becomes a mask."""
        names = [g["name"] for g in self.param_groups]
        if sorted(tensors_dict) != sorted(names):
            raise ValueError(f"GaussianAdam.append: rows for {sorted(tensors_dict)}, the groups are {names}")
        counts = {int(t.shape[0]) for t in tensors_dict.values()}
        if len(counts) != 1:
            raise ValueError("GaussianAdam.append: the new tensors must share their row count")
        n_new = counts.pop()
        P = int(self.param_groups[0]["params"][0].shape[0])
        out = {}
        with torch.no_grad():
            for g in self.param_groups:
                p = g["params"][0]
                ext = tensors_dict[g["name"]].detach().to(device=p.device, dtype=p.dtype)
                st = self.state.get(g["name"])
                if st is not None:
                    st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
                    st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
                out[g["name"]] = self._rewrap(g, torch.cat((p.detach(), ext), dim=0))
        if self.rows is not None and self.rows[1] != P:
            live = self._live(P, self.model._xyz.device)
            self.row_mask, self.rows = live.to(torch.uint8), None
        if self.row_mask is not None:
            self.row_mask = torch.cat((self.row_mask, torch.ones(n_new, dtype=torch.uint8, device=self.row_mask.device)))
        if self.rows is not None:
            self.rows = (self.rows[0], P + n_new)
        return out

    def install(self, tensors: Dict[str, torch.Tensor], moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]],
                row_mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Install what a densify or a fused prune moved (GaussianModel.densify_and_prune / prune_points): every group takes
        its new tensor as a new nn.Parameter (so a render cache sees new geometry) and, where it has state, its moved moments.
        row_mask: the moved row selection (kept rows their byte, new rows 1), given iff the optimiser selects rows; a row
        range becomes that mask -- append's rule for a range that does not end at the last row, applied to every range, so
        that no count has to come back from the device.  -> the entries of `tensors` that belong to no group."""
        names = {g["name"] for g in self.param_groups}
        if (self.row_mask is not None or self.rows is not None) != (row_mask is not None):
            raise ValueError("GaussianAdam.install: a moved row mask is needed iff the optimiser selects rows")
        with torch.no_grad():
            for g in self.param_groups:
                n = g["name"]
                new = self._rewrap(g, tensors[n].detach())
                if n in self.state:
                    m, v = moments[n]
                    if m.shape != new.shape or v.shape != new.shape:
                        raise ValueError(f"GaussianAdam.install: {n}: moments of shape {tuple(m.shape)} for {tuple(new.shape)}")
                    self.state[n] = dict(exp_avg=m, exp_avg_sq=v)
        if row_mask is not None:
            self.row_mask, self.rows = row_mask.to(torch.uint8).contiguous(), None
        return {n: t for n, t in tensors.items() if n not in names}

    def replace(self, name: str, tensor: torch.Tensor) -> nn.Parameter:
        """A new tensor for one group with its moments reset to zero (reference replace_tensor_to_optimizer)."""
        for g in self.param_groups:
            if g["name"] == name:
                p = g["params"][0]
                if int(tensor.shape[0]) != int(p.shape[0]):
                    raise ValueError(f"GaussianAdam.replace: {tensor.shape[0]} rows for a group of {p.shape[0]}")
                new = self._rewrap(g, tensor.detach().to(device=p.device, dtype=p.dtype).clone())
                if name in self.state:
                    self.state[name] = dict(exp_avg=torch.zeros_like(new), exp_avg_sq=torch.zeros_like(new))
                return new
        raise ValueError(f"GaussianAdam.replace: no group {name!r}")


def refit(model, cameras, targets, *, iters: int, lambda_dssim: float = 0.2, pipe=None, background=None,
          views_per_step: int = 1, densify=None) -> torch.Tensor:
    """The plain fit loop of a model whose optimiser is set up (training_setup, finetune_setup or inpaint_setup(opt=...)):
    per step update_learning_rate, render the next `views_per_step` cameras (round robin; render_batch for more than one),
    photometric_loss against their targets, backward, optimizer.step(), zero_grad.  targets: [V,3,H,W] or a sequence of
    [3,H,W], one per camera.  -> the per-step losses [iters] on the device (one read-back for the caller).
    densify: None (no densification: the loop above and nothing else) or a gsplat_attack.densify.DensifyParams: the reference's
    schedule (that of the original 3D Gaussian Splatting training loop) -- oneupSHdegree every sh_degree_interval iterations at the top of the loop; after the backward, while
    iteration < densify_until_iter, add_densification_stats (with the radii) every iteration, densify_and_prune every
    densification_interval iterations past densify_from_iter (max_screen_size once past opacity_reset_interval), reset_opacity
    every opacity_reset_interval; then the step.  Iterations count from 1."""
    from .image_loss import photometric_loss
    from .renderer import PipelineParams, render, render_batch
    if getattr(model, "optimizer", None) is None:
        raise ValueError("refit: the model has no optimiser; call training_setup, finetune_setup or inpaint_setup(opt=...)")
    cameras = list(cameras)
    V, k = len(cameras), int(views_per_step)
    if V == 0 or len(targets) != V or k < 1:
        raise ValueError(f"refit: {V} cameras, {len(targets)} targets, views_per_step={k}")
    dev = model._xyz.device
    pipe = pipe if pipe is not None else PipelineParams(skip_objects=True)
    bg = background if background is not None else torch.zeros(3, device=dev)
    losses = torch.zeros(int(iters), device=dev)
    for it in range(int(iters)):
        model.update_learning_rate(it + 1)
        ids = [(it * k + j) % V for j in range(k)]
        gt = torch.stack([targets[i] for i in ids]).to(dev)
        if densify is not None:
            sh_up, dens, reset, size = densify.actions(it + 1)
            if sh_up:
                model.oneupSHdegree()
        if k == 1:
            out = render(cameras[ids[0]], model, pipe, bg)
            img = out["render"][None]
        else:
            out = render_batch([cameras[i] for i in ids], model, pipe, bg)
            img = out["render"]
        loss = photometric_loss(img, gt, lambda_dssim)
        loss.backward()
        losses[it] = loss.detach()
        if densify is not None and it + 1 < densify.densify_until_iter:
            with torch.no_grad():
                model.add_densification_stats(out["viewspace_points"], None, radii=out["radii"])
                if dens:
                    model.densify_and_prune(densify.densify_grad_threshold, densify.min_opacity,
                                            densify.extent if densify.extent is not None else model.spatial_lr_scale, size,
                                            N=densify.N, seed=densify.seed, screen_prune=densify.screen_prune)
                if reset:
                    model.reset_opacity()
        model.optimizer.step()
        model.optimizer.zero_grad()
    return losses

"""Attribute container with the names/shapes/activations the render boundary and
the PGD step functions read.

Counterpart of the getters of the reference's ``scene/gaussian_model.py:24-39,97-124``
(seven parameter tensors + exp / sigmoid / normalize / cat activations).  The fitting set-ups
(training_setup, finetune_setup, the tail of inpaint_setup, update_learning_rate: :160-214,350-375) put a
gsplat_attack.optim.GaussianAdam on the model; adaptive density control (:413-416, :591-712: add_densification_stats,
densify_and_prune, prune_points, reset_opacity, oneupSHdegree) runs through diff_gaussian_rasterization.densify_ops on a
device and through the tensor ops of gsplat_attack.densify on the host.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

NUM_OBJECTS = 16  # scene/gaussian_model.py:52


class GaussianModel:
    def __init__(self, sh_degree: int = 3):
        self.max_sh_degree = sh_degree
        self.active_sh_degree = sh_degree      # load_ply sets active = max (scene/gaussian_model.py:467)
        self.num_objects = NUM_OBJECTS
        self.spatial_lr_scale = 1.0            # scales the position learning rates (scene/gaussian_model.py:56,131)
        self.percent_dense = 0.0
        self.optimizer = None
        self.xyz_scheduler_args = None
        e = torch.empty(0)
        self._xyz = e
        self._features_dc = e
        self._features_rest = e
        self._scaling = e
        self._rotation = e
        self._opacity = e
        self._objects_dc = e
        # the densification statistics (reference :57-59,176-177): created by the set-ups, reset by a densify
        self.xyz_gradient_accum = e
        self.denom = e
        self.max_radii2D = e
        self.densify_count = 0                 # the default seed of densify_and_prune's keyed normals: a fit repeats

    # ---- construction -------------------------------------------------
    @classmethod
    def from_tensors(cls, xyz, features_dc, features_rest, scaling, rotation, opacity, objects_dc=None,
                     sh_degree: int = 3, device=None, requires_grad: bool = True) -> "GaussianModel":
        """Raw (pre-activation) tensors with the load_ply layout (scene/gaussian_model.py:459-467):
        xyz [P,3], features_dc [P,1,3], features_rest [P,K-1,3], scaling (log) [P,3],
        rotation (w,x,y,z un-normalised) [P,4], opacity (logit) [P,1], objects_dc [P,1,16]."""
        m = cls(sh_degree)
        P = xyz.shape[0]
        if objects_dc is None:
            objects_dc = torch.zeros(P, 1, NUM_OBJECTS)

        def par(t):
            t = t.detach().to(torch.float32)
            if device is not None:
                t = t.to(device)
            return nn.Parameter(t.contiguous().clone(), requires_grad=requires_grad)
        m._xyz = par(xyz)
        m._features_dc = par(features_dc)
        m._features_rest = par(features_rest)
        m._scaling = par(scaling)
        m._rotation = par(rotation)
        m._opacity = par(opacity)
        m._objects_dc = par(objects_dc)
        return m

    @classmethod
    def create_from_pcd(cls, points, colors, sh_degree: int = 3, device="cpu", generator=None,
                        spatial_lr_scale: float = 1.0) -> "GaussianModel":
        """Initial model from a sparse point cloud (reference scene/gaussian_model.py:130-158): DC colour = RGB2SH(rgb),
        higher bands 0, isotropic log-scale = log sqrt(mean squared distance to the 3 nearest neighbours)
        (``simple_knn._C.distCUDA2`` -- the HIP kernel on a device, clamped at 1e-7), identity rotations, opacity
        logit(0.1), random object features RGB2SH(U[0,1)).  points [P,3], colors [P,3] in [0,1] (array-likes).
        spatial_lr_scale (the reference's second argument, the scene's camera extent) is kept for training_setup."""
        from simple_knn._C import distCUDA2
        from .sh import RGB2SH
        xyz = torch.as_tensor(points, dtype=torch.float32).to(device).contiguous()
        rgb = torch.as_tensor(colors, dtype=torch.float32).to(device)
        P = xyz.shape[0]
        K = (sh_degree + 1) ** 2
        dist2 = torch.clamp_min(distCUDA2(xyz), 1e-7)
        scales = torch.log(torch.sqrt(dist2))[:, None].repeat(1, 3)
        rots = torch.zeros(P, 4, device=xyz.device)
        rots[:, 0] = 1.0
        opac = torch.full((P, 1), 0.1, device=xyz.device)
        opac = torch.log(opac / (1.0 - opac))                            # inverse_sigmoid, utils/general_utils.py:18-19
        objs = RGB2SH(torch.rand(P, NUM_OBJECTS, generator=generator).to(xyz.device))[:, None, :]
        m = cls.from_tensors(xyz, RGB2SH(rgb)[:, None, :], torch.zeros(P, K - 1, 3, device=xyz.device), scales, rots,
                             opac, objs, sh_degree=sh_degree, device=xyz.device)
        m.spatial_lr_scale = float(spatial_lr_scale)
        return m

    def parameters(self):
        return [self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self._objects_dc]

    def named_parameters(self):
        return dict(xyz=self._xyz, f_dc=self._features_dc, f_rest=self._features_rest, scaling=self._scaling,
                    rotation=self._rotation, opacity=self._opacity, objects_dc=self._objects_dc)

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None

    _PARAM_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_objects_dc")

    # ---- scene surgery used by the attack set-up (scene/gaussian_model.py:216-262) ------------------------------
    def removal_setup(self, mask3d: torch.Tensor) -> None:
        """Keep the Gaussians NOT selected by mask3d (reference :216-241).  As in the reference the survivors are
        re-wrapped in nn.Parameter, whose default requires_grad=True wins."""
        keep = ~mask3d.bool().reshape(-1)
        for n in self._PARAM_ATTRS:
            setattr(self, n, nn.Parameter(getattr(self, n)[keep].detach().clone()))

    # ---- the fitting set-ups (scene/gaussian_model.py:160-214,350-375) ------------------------------------------------
    def _setup_optimizer(self, opt, row_mask=None, rows=None) -> None:
        from .optim import GaussianAdam, get_expon_lr_func, reference_groups
        self.percent_dense = opt.percent_dense
        self.optimizer = GaussianAdam(self, reference_groups(opt, self.spatial_lr_scale), eps=1e-15, row_mask=row_mask, rows=rows)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=opt.position_lr_init * self.spatial_lr_scale,
                                                    lr_final=opt.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=opt.position_lr_delay_mult,
                                                    max_steps=opt.position_lr_max_steps)
        self._reset_densification_stats()

    def _reset_densification_stats(self) -> None:
        P, dev = int(self._xyz.shape[0]), self._xyz.device
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        self.max_radii2D = torch.zeros((P,), device=dev)

    def training_setup(self, opt) -> None:
        """The optimiser of a full fit (reference :160-179): Adam(lr=0, eps=1e-15) over the seven groups xyz, f_dc, f_rest,
        opacity, scaling, rotation, obj_dc with the rates of `opt` (gsplat_attack.optim.OptimizationParams), and the
        position schedule.  Afterwards self.optimizer is a gsplat_attack.optim.GaussianAdam."""
        self._setup_optimizer(opt)

    def finetune_setup(self, opt, mask3d: torch.Tensor) -> None:
        """Move only the Gaussians mask3d selects (reference :181-214); _objects_dc is frozen.  The reference registers
        gradient hooks that multiply every gradient by mask3d and steps all rows; here the mask is the optimiser's row
        mask and the other rows are neither read nor written.  The two agree: a row whose gradient is always zero and
        whose moments start at zero never moves under Adam (m' = v' = 0, 0 / (0 + eps) = 0)."""
        mask = mask3d.detach().reshape(-1)
        if mask.numel() != self._xyz.shape[0]:
            raise ValueError(f"finetune_setup: mask of {mask.numel()} entries for {self._xyz.shape[0]} Gaussians")
        self._objects_dc.requires_grad = False
        self._setup_optimizer(opt, row_mask=mask != 0)

    def update_learning_rate(self, iteration: int) -> float:
        """Set the xyz group's learning rate from the position schedule and return it (reference :369-375)."""
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                lr = self.xyz_scheduler_args(iteration)
                group["lr"] = lr
                return lr

    def inpaint_setup(self, mask3d: torch.Tensor, k: int = 5, opt=None) -> torch.Tensor:
        """Fill the hole a removal leaves (reference scene/gaussian_model.py:264-348): the Gaussians NOT selected by mask3d
        stay, first and in their order; behind them comes one new Gaussian per removed one, in the removed rows' order,
        whose seven raw attributes (positions, logit opacities, log scales, raw quaternions, both SH blocks, object
        features) are each the mean over the k remaining Gaussians nearest to the removed one's position.  All seven
        tensors are re-wrapped in nn.Parameter.  -> the bool mask [P'] of the new rows.

        On a HIP device the neighbours come from gsr_knn_query and the means from gsr_knn_gather_mean
        (diff_gaussian_rasterization.knn_ops): nothing goes to the host, where the reference builds a scipy KDTree and takes
        all seven tensors through numpy.  The mean is the float32 sum in rank order divided by the count.

        Deviations from the reference: ties between equidistant neighbours go to the lower index (KDTree's choice is
        arbitrary); with fewer than k remaining Gaussians the mean is over those there are, and with none a ValueError is
        raised (the reference fails with an index error); the reference's distance_threshold / max_distance_threshold
        arguments do not exist here, because the reference never reads them.

        opt (gsplat_attack.optim.OptimizationParams, optional): also set up the optimiser of the reference's tail
        (:350-367), with the new rows as its row range.  Deviation: in the reference every row ends up trainable, because
        nn.Parameter re-enables the gradient of the concatenated tensors, although its comment says "Only the new points
        will have gradients"; here the comment's intent is the behaviour, and setting `model.optimizer.rows = None`
        restores the reference's.  Without opt no optimiser is set up."""
        from diff_gaussian_rasterization import knn_ops
        removed = mask3d.bool().reshape(-1).to(self._xyz.device)
        if removed.numel() != self._xyz.shape[0]:
            raise ValueError(f"inpaint_setup: mask of {removed.numel()} entries for {self._xyz.shape[0]} Gaussians")
        keep = ~removed
        n_new = int(removed.sum())
        if n_new and n_new == removed.numel():
            raise ValueError("inpaint_setup: no Gaussian remains to fill the hole from")
        with torch.no_grad():
            rest = [getattr(self, n)[keep].detach() for n in self._PARAM_ATTRS]
            if n_new:
                idx, _ = knn_ops.knn_query(rest[0], self._xyz.detach()[removed], k=k, exclude_self=False)
                new = knn_ops.gather_mean(idx, rest)
            else:
                new = [r[:0] for r in rest]
            for n, r, w in zip(self._PARAM_ATTRS, rest, new):
                setattr(self, n, nn.Parameter(torch.cat([r, w.to(r.dtype)]).detach().clone()))
        new_mask = torch.zeros(self._xyz.shape[0], dtype=torch.bool, device=self._xyz.device)
        new_mask[self._xyz.shape[0] - n_new:] = n_new > 0
        if opt is not None:
            self._setup_optimizer(opt, rows=(self._xyz.shape[0] - n_new, self._xyz.shape[0]))
        return new_mask

    # ---- adaptive density control (scene/gaussian_model.py:413-416,591-712) ------------------------------------------------
    def oneupSHdegree(self) -> None:
        """reference :126-128"""
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def reset_opacity(self) -> None:
        """Clamp every opacity at 0.01 and reset the opacity group's moments (reference :413-416, tensor ops as written
        there, through GaussianAdam.replace)."""
        op = self.get_opacity.detach()
        x = torch.min(op, torch.ones_like(op) * 0.01)
        new = torch.log(x / (1 - x))                                         # inverse_sigmoid, utils/general_utils.py:18-19
        if self.optimizer is not None:
            self.optimizer.replace("opacity", new)
        else:
            self._opacity = nn.Parameter(new, requires_grad=self._opacity.requires_grad)

    def _stats_ready(self) -> None:
        if self.xyz_gradient_accum.shape[0] != self._xyz.shape[0] or self.xyz_gradient_accum.device != self._xyz.device:
            self._reset_densification_stats()

    def add_densification_stats(self, viewspace_point_tensor, update_filter, radii=None) -> None:
        """xyz_gradient_accum[f] += |grad[f, :2]|, denom[f] += 1 (reference :710-712) and, with radii, max_radii2D[f] =
        max(max_radii2D[f], radii[f]) (the line of the reference's training loop), f = update_filter.  viewspace_point_tensor:
        the render's `viewspace_points` leaf after the backward ([P,3], or a batch's [B,P,3] with update_filter and radii
        [B,P]: the views are taken in order) or the gradient itself.  update_filter None: radii > 0.  One launch on a device."""
        g = viewspace_point_tensor.grad if getattr(viewspace_point_tensor, "grad", None) is not None else viewspace_point_tensor
        g = g.detach()
        if update_filter is None and radii is None:
            raise ValueError("add_densification_stats: neither update_filter nor radii")
        self._stats_ready()
        if g.is_cuda:
            from diff_gaussian_rasterization import densify_ops
            densify_ops.stats_(g.to(torch.float32).contiguous(), self.xyz_gradient_accum, self.denom, radii, update_filter,
                               self.max_radii2D if radii is not None else None)
            return
        if g.dim() == 2:
            g = g[None]
        B = g.shape[0]
        rad = None if radii is None else radii.reshape(B, -1)
        flt = (rad > 0) if update_filter is None else (update_filter.reshape(B, -1) != 0)
        for b in range(B):                              # csrc/gsr_densify.h: sqrt(gx gx + gy gy), every operation rounded once
            f = flt[b]
            gx, gy = g[b, :, 0].to(torch.float32), g[b, :, 1].to(torch.float32)
            norm = torch.from_numpy(np.sqrt((gx * gx + gy * gy).numpy()))      # numpy's root rounds once; torch's vectorised one need not
            self.xyz_gradient_accum[f] += norm[f][:, None]
            self.denom[f] += 1
            if rad is not None:
                self.max_radii2D[f] = torch.max(self.max_radii2D[f], rad[b][f].to(torch.float32))

    def _groups(self):
        """[(group name, attribute)] in the optimiser's order, or the reference's when there is none"""
        from .optim import GROUP_ATTRS
        if self.optimizer is None:
            return list(GROUP_ATTRS)
        attrs = dict(GROUP_ATTRS)
        named = [(g["name"], attrs[g["name"]]) for g in self.optimizer.param_groups]
        return named + [(n, a) for n, a in GROUP_ATTRS if n not in dict(named)]

    def _install(self, new: dict, moments: dict, mask_out) -> None:
        if self.optimizer is not None:
            rest = self.optimizer.install(new, moments, mask_out)
        else:
            rest = new
        attrs = dict(self._groups())
        for name, data in rest.items():                 # tensors outside the optimiser's groups
            old = getattr(self, attrs[name])
            setattr(self, attrs[name], nn.Parameter(data.contiguous(), requires_grad=old.requires_grad))

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, *, N: int = 2, seed=None, normals=None,
                          screen_prune: bool = False):
        """Clone, split and prune in one pass (reference :694-708 with :652-692; the contract, its stated deviations and the
        non-finite rules are in csrc/gsr_densify.h).  As in the reference the screen-size test is inert and a truthy
        max_screen_size only switches on the world-size prune (max scale > 0.1 extent); screen_prune=True (an extension)
        also prunes original rows whose max_radii2D, accumulated before the call, exceeds max_screen_size.  normals: None
        (keyed by seed; seed None: the model's densify_count, so a fit repeats) or [P,N,3] standard normals.  Parameters,
        Adam moments and the optimiser's row selection follow their rows; new rows have zero moments and move.  The
        statistics are reset.  -> (origin, kind) int32 [P']: the source row, and 0 keep, 1 clone, 2 + j child j."""
        from . import densify as DZ
        if self.optimizer is None and self.percent_dense == 0.0:
            raise ValueError("densify_and_prune: percent_dense is not set; call a set-up with an OptimizationParams first")
        self._stats_ready()
        if seed is None:
            seed = self.densify_count
        self.densify_count += 1
        groups = self._groups()
        opt = self.optimizer
        state = {} if opt is None else opt.state
        live = None if opt is None else opt._live(int(self._xyz.shape[0]), self._xyz.device)
        with torch.no_grad():
            if self._xyz.is_cuda:
                from diff_gaussian_rasterization import densify_ops as DO
                pl = DO.plan(self.xyz_gradient_accum, self.denom, self._scaling, self._opacity, max_grad=max_grad, min_opacity=min_opacity,
                             extent=extent, percent_dense=self.percent_dense, max_screen_size=max_screen_size, N=N,
                             screen_prune=screen_prune, max_radii=self.max_radii2D)
                role = dict(xyz=DO.XYZ, scaling=DO.SCALE)
                items = []
                for name, attr in groups:
                    st = state.get(name)
                    items.append((getattr(self, attr).detach(), None if st is None else st["exp_avg"], None if st is None else st["exp_avg_sq"],
                                  role.get(name, DO.COPY)))
                outs, mask_out, origin, kind = DO.apply(pl, items, self._rotation.detach(), seed=seed, normals=normals, row_mask=live)
                new = {name: o[0] for (name, _), o in zip(groups, outs)}
                moments = {name: (o[1], o[2]) for (name, _), o in zip(groups, outs) if o[1] is not None}
            else:
                thr = DZ.thresholds(max_grad, min_opacity, extent, self.percent_dense, N, max_screen_size, screen_prune)
                keep, clone, kids = DZ.classify(self.xyz_gradient_accum, self.denom, self._scaling.detach(), self._opacity.detach(),
                                                self.max_radii2D, thr, max_screen_size, screen_prune)
                P = int(self._xyz.shape[0])
                if normals is None:
                    z = torch.zeros(P, N, 3)
                    rows = kids.nonzero().reshape(-1)
                    z[rows] = torch.from_numpy(DZ.keyed_normals(seed, rows.numpy(), N))
                else:
                    z = normals.to(torch.float32)
                tensors = {name: getattr(self, attr).detach() for name, attr in groups}
                moms = {name: (state[name]["exp_avg"], state[name]["exp_avg_sq"]) for name, _ in groups if state.get(name) is not None}
                new, moments, origin, kind = DZ.move_host(tensors, moms, keep, clone, kids, N, thr["c"], z)
                mask_out = None
                if live is not None:
                    mask_out = torch.ones(origin.numel(), dtype=torch.uint8)
                    nk = int(keep.sum())
                    mask_out[:nk] = live[keep].to(torch.uint8)
            self._install(new, moments, mask_out)
        self._reset_densification_stats()
        return origin, kind

    def prune_points(self, mask: torch.Tensor) -> None:
        """Remove the rows mask selects (reference :591-606): parameters, moments, the row selection and the three
        statistics follow their rows.  On a device: the fused prune of gsr_densify_apply (no clone, no split)."""
        mask = mask.detach().reshape(-1).bool().to(self._xyz.device)
        P = int(self._xyz.shape[0])
        if mask.numel() != P:
            raise ValueError(f"prune_points: mask of {mask.numel()} entries for {P} Gaussians")
        self._stats_ready()
        stats = dict(xyz_gradient_accum=self.xyz_gradient_accum, denom=self.denom, max_radii2D=self.max_radii2D)
        with torch.no_grad():
            if not self._xyz.is_cuda:
                keep = ~mask
                if self.optimizer is not None:
                    self.optimizer.prune(keep)
                    rest = [a for n, a in self._groups() if n not in {g["name"] for g in self.optimizer.param_groups}]
                else:
                    rest = [a for _, a in self._groups()]
                for a in rest:
                    old = getattr(self, a)
                    setattr(self, a, nn.Parameter(old.detach()[keep].clone(), requires_grad=old.requires_grad))
                for n, t in stats.items():
                    setattr(self, n, t[keep])
                return
            from diff_gaussian_rasterization import densify_ops as DO
            pl = DO.plan_prune(mask)
            groups = self._groups()
            opt = self.optimizer
            state = {} if opt is None else opt.state
            live = None if opt is None else opt._live(P, self._xyz.device)
            items = []
            for name, attr in groups:
                st = state.get(name)
                items.append((getattr(self, attr).detach(), None if st is None else st["exp_avg"], None if st is None else st["exp_avg_sq"], DO.COPY))
            items += [(t, None, None, DO.COPY) for t in stats.values()]
            outs, mask_out, _, _ = DO.apply(pl, items, self._rotation.detach(), row_mask=live, want_origin=False)
            new = {name: o[0] for (name, _), o in zip(groups, outs)}
            moments = {name: (o[1], o[2]) for (name, _), o in zip(groups, outs) if o[1] is not None}
            self._install(new, moments, mask_out)
            for n, o in zip(stats, outs[len(groups):]):
                setattr(self, n, o[0])

    def concat_setup(self, feature_name: str, tensor_to_concat: torch.Tensor, requires_grad: bool) -> None:
        """Append rows to one attribute and re-wrap it (reference :243-262)."""
        cur = getattr(self, f"_{feature_name}")
        cat = torch.cat((cur, tensor_to_concat.to(cur.device)), dim=0).detach().clone().requires_grad_(requires_grad)
        setattr(self, f"_{feature_name}", nn.Parameter(cat, requires_grad=requires_grad))

    def clone(self) -> "GaussianModel":
        m = GaussianModel(self.max_sh_degree)
        m.active_sh_degree = self.active_sh_degree
        m.spatial_lr_scale = self.spatial_lr_scale
        for n in self._PARAM_ATTRS:
            p = getattr(self, n)
            setattr(m, n, nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad))
        return m

    def save_ply(self, path: str) -> None:
        from .ply import save_gaussians
        save_gaussians(self, path)

    @classmethod
    def load_ply(cls, path: str, sh_degree: int = 3, device=None) -> "GaussianModel":
        from .ply import load_gaussians
        return load_gaussians(path, sh_degree, device)

    # ---- getters (scene/gaussian_model.py:97-124) ---------------------
    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_objects(self):
        return self._objects_dc

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier: float = 1.0):
        """scene/gaussian_model.py:25-29 with utils/general_utils.py:64-110 (which re-normalises
        the raw quaternion inside build_rotation): packed (xx,xy,xz,yy,yz,zz)."""
        q = self._rotation / self._rotation.norm(dim=1, keepdim=True)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
        L = R * (scaling_modifier * self.get_scaling)[:, None, :]
        S = L @ L.transpose(1, 2)
        return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)

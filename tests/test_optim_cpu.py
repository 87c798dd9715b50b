"""gsplat_attack.optim.GaussianAdam and the three fitting set-ups of GaussianModel on the CPU (the tensor-op formulation of the
step; the kernel is held to the same arithmetic bit for bit in tests/test_gpu_adam.py): against a torch.optim.Adam built
exactly as the reference's training_setup builds it, the reference's gradient-hook formulation of finetune_setup, and the
reference's state surgery semantics.  No GPU."""
import numpy as np
import pytest
import torch

import adam_cases as AC
from gsplat_attack.gaussian_model import GaussianModel
from gsplat_attack.optim import GROUP_ATTRS, GaussianAdam, OptimizationParams

P, STEPS = 300, 20
NAMES = [n for n, _ in GROUP_ATTRS]
ATTRS = dict(GROUP_ATTRS)


def make_model(seed=0, P=P):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return GaussianModel.from_tensors(r(P, 3), r(P, 1, 3), 0.1 * r(P, 15, 3), r(P, 3) - 3.0, r(P, 4), r(P, 1), r(P, 1, 16), device="cpu")


def grads(model, steps=STEPS, seed=1):
    """pre-drawn gradients per step and group: a steady part plus noise, independent of the parameters"""
    g = torch.Generator().manual_seed(seed)
    steady = {n: torch.randn(getattr(model, ATTRS[n]).shape, generator=g) for n in NAMES}
    return [{n: steady[n] + torch.randn(steady[n].shape, generator=g) for n in NAMES} for _ in range(steps)]


def reference_adam(model, opt, scale=1.0):
    """torch.optim.Adam exactly as reference scene/gaussian_model.py:165-175 builds it, on clones of the model's tensors"""
    ps = {n: torch.nn.Parameter(getattr(model, ATTRS[n]).detach().clone(), requires_grad=getattr(model, ATTRS[n]).requires_grad) for n in NAMES}
    groups = [
        {"params": [ps["xyz"]], "lr": opt.position_lr_init * scale, "name": "xyz"},
        {"params": [ps["f_dc"]], "lr": opt.feature_lr, "name": "f_dc"},
        {"params": [ps["f_rest"]], "lr": opt.feature_lr / 20.0, "name": "f_rest"},
        {"params": [ps["opacity"]], "lr": opt.opacity_lr, "name": "opacity"},
        {"params": [ps["scaling"]], "lr": opt.scaling_lr, "name": "scaling"},
        {"params": [ps["rotation"]], "lr": opt.rotation_lr, "name": "rotation"},
        {"params": [ps["obj_dc"]], "lr": opt.feature_lr, "name": "obj_dc"},
    ]
    return ps, torch.optim.Adam(groups, lr=0.0, eps=1e-15)


def set_grads(model, gs, mult=None):
    for n in NAMES:
        p = getattr(model, ATTRS[n])
        if p.requires_grad:
            p.grad = gs[n].clone() if mult is None else gs[n] * mult.reshape((-1,) + (1,) * (gs[n].dim() - 1))


def within_bound(ours, theirs, steps, lr, what, rows=None):
    a, b = ours.detach().double(), theirs.detach().double()
    if rows is not None:
        a, b = a[rows], b[rows]
    tol = AC.trajectory_bound(steps, float(torch.maximum(a.abs(), b.abs()).max()), lr)
    err = float((a - b).abs().max())
    assert err <= tol, f"{what}: error {err:.3e}, bound {tol:.3e}"
    return err / tol


def test_groups_and_defaults():
    o = OptimizationParams()
    assert (o.position_lr_init, o.position_lr_final, o.position_lr_delay_mult, o.position_lr_max_steps) == (0.00016, 0.0000016, 0.01, 30000)
    assert (o.feature_lr, o.opacity_lr, o.scaling_lr, o.rotation_lr, o.percent_dense) == (0.0025, 0.05, 0.005, 0.001, 0.01)
    m = make_model()
    assert m.spatial_lr_scale == 1.0 and m.optimizer is None
    m.spatial_lr_scale = 2.5
    m.training_setup(o)
    assert isinstance(m.optimizer, GaussianAdam) and m.percent_dense == 0.01
    assert [g["name"] for g in m.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "obj_dc"]
    assert [g["lr"] for g in m.optimizer.param_groups] == [0.00016 * 2.5, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001, 0.0025]
    for g in m.optimizer.param_groups:
        assert g["params"][0] is getattr(m, ATTRS[g["name"]])
    assert m.optimizer.eps == 1e-15 and m.optimizer.betas == (0.9, 0.999) and m.optimizer.state == {}
    assert m.clone().spatial_lr_scale == 2.5


def test_training_setup_against_torch_adam_over_20_steps():
    opt = OptimizationParams()
    m = make_model()
    m.spatial_lr_scale = 1.7
    ps, ref = reference_adam(m, opt, 1.7)
    m.training_setup(opt)
    start = {n: getattr(m, ATTRS[n]).detach().clone() for n in NAMES}
    worst = 0.0
    for it, gs in enumerate(grads(m)):
        lr = m.update_learning_rate(it + 1)
        ref.param_groups[0]["lr"] = lr
        set_grads(m, gs)
        for n in NAMES:
            ps[n].grad = gs[n].clone()
        m.optimizer.step()
        ref.step()
        m.optimizer.zero_grad()
        assert all(getattr(m, ATTRS[n]).grad is None for n in NAMES)
    assert m.optimizer.step_count == STEPS
    for g in m.optimizer.param_groups:
        n = g["name"]
        moved = (getattr(m, ATTRS[n]).detach() - start[n]).abs()
        assert float(moved.min()) > 0 and float(moved.median()) > 0.25 * STEPS * g["lr"], n   # a steady gradient: the elements travel
        worst = max(worst, within_bound(getattr(m, ATTRS[n]), ps[n], STEPS, max(g["lr"], opt.position_lr_init * 1.7), n))
        st = ref.state[ps[n]]
        assert torch.allclose(m.optimizer.state[n]["exp_avg"], st["exp_avg"], rtol=1e-5, atol=1e-7)
        # 1 - b2 is formed from the float32 b2 (csrc/gsr_adam.h): 1 - 0.999f = 0.00099998713, 1.29e-5 relative below torch's 0.001
        assert torch.allclose(m.optimizer.state[n]["exp_avg_sq"], st["exp_avg_sq"], rtol=1e-4, atol=1e-9)
    print(f"GaussianAdam vs torch.optim.Adam, {STEPS} steps: worst error / bound {worst:.3f}")


def test_finetune_setup_against_the_gradient_hook_formulation():
    """the reference multiplies every gradient by mask3d in hooks and steps all rows with a plain Adam"""
    opt = OptimizationParams()
    m = make_model(seed=3)
    mask = torch.zeros(P, dtype=torch.bool)
    mask[torch.randperm(P, generator=torch.Generator().manual_seed(5))[:90]] = True
    m.finetune_setup(opt, mask[:, None].float())                 # the reference's mask3d is [P, 1]
    assert not m._objects_dc.requires_grad and m.optimizer.row_mask.dtype == torch.uint8 and int(m.optimizer.row_mask.sum()) == 90
    ps, ref = reference_adam(m, opt)
    assert not ps["obj_dc"].requires_grad
    start = {n: getattr(m, ATTRS[n]).detach().clone() for n in NAMES}
    for gs in grads(m, seed=7):
        set_grads(m, gs)                                          # ours: the whole gradient, the optimiser selects the rows
        for n in NAMES[:-1]:
            ps[n].grad = gs[n] * mask.reshape((-1,) + (1,) * (gs[n].dim() - 1)).float()
        m.optimizer.step()
        ref.step()
        m.optimizer.zero_grad()
    assert torch.equal(m._objects_dc, start["obj_dc"]) and "obj_dc" not in m.optimizer.state
    for g in m.optimizer.param_groups[:-1]:
        n = g["name"]
        p = getattr(m, ATTRS[n]).detach()
        assert torch.equal(p[~mask], start[n][~mask]), n          # bit for bit
        assert torch.equal(ps[n].detach()[~mask], start[n][~mask]), n          # ... as in the reference's formulation
        assert not m.optimizer.state[n]["exp_avg"][~mask].any() and not m.optimizer.state[n]["exp_avg_sq"][~mask].any()
        assert (p[mask] != start[n][mask]).all(), n
        within_bound(p, ps[n], STEPS, g["lr"], n, rows=mask)


def test_a_group_without_gradient_is_left_out_with_its_state_untouched():
    m = make_model()
    m.training_setup(OptimizationParams())
    gs = grads(m, steps=2)
    set_grads(m, gs[0])
    m.optimizer.step()
    kept = {k: v.clone() for k, v in m.optimizer.state["opacity"].items()}
    before = m._opacity.detach().clone()
    set_grads(m, gs[1])
    m._opacity.grad = None
    m.optimizer.step()
    assert torch.equal(m._opacity, before) and all(torch.equal(kept[k], m.optimizer.state["opacity"][k]) for k in kept)
    assert m.optimizer.step_count == 2
    m.optimizer.zero_grad(set_to_none=False)
    assert all(p.grad is None or not p.grad.any() for p in m.parameters()) and m._xyz.grad is not None
    m.optimizer.zero_grad()
    m.optimizer.step()                                            # nothing has a gradient: no step is counted
    assert m.optimizer.step_count == 2


def test_update_learning_rate_sets_only_xyz():
    from gsplat_attack.optim import get_expon_lr_func
    opt = OptimizationParams()
    m = make_model()
    m.spatial_lr_scale = 3.0
    m.training_setup(opt)
    others = [g["lr"] for g in m.optimizer.param_groups[1:]]
    want = get_expon_lr_func(0.00016 * 3.0, 0.0000016 * 3.0, lr_delay_mult=0.01, max_steps=30000)
    for it in (1, 100, 15000, 30000, 40000):
        lr = m.update_learning_rate(it)
        assert lr == want(it) == m.optimizer.param_groups[0]["lr"]
        assert [g["lr"] for g in m.optimizer.param_groups[1:]] == others
    assert abs(m.update_learning_rate(30000) - 0.0000016 * 3.0) < 1e-18
    m.optimizer.param_groups[2]["lr"] = 0.5                        # code that sets group['lr'] works
    assert m.optimizer.param_groups[2]["lr"] == 0.5


def _stepped_model(mask=None, rows=None, steps=3):
    m = make_model(seed=11)
    m._setup_optimizer(OptimizationParams(), row_mask=mask, rows=rows)
    for gs in grads(m, steps=steps, seed=13):
        set_grads(m, gs)
        m.optimizer.step()
        m.optimizer.zero_grad()
    return m


def test_prune_append_and_replace_follow_the_reference_semantics():
    mask = torch.arange(P) % 3 == 0
    m = _stepped_model(mask=mask)
    o = m.optimizer
    old_p = {n: getattr(m, ATTRS[n]).detach().clone() for n in NAMES}
    old_s = {n: {k: v.clone() for k, v in o.state[n].items()} for n in NAMES}
    keep = torch.rand(P, generator=torch.Generator().manual_seed(2)) > 0.25
    out = o.prune(keep)                                            # _prune_optimizer: state[mask], Parameter(param[mask])
    K = int(keep.sum())
    for g in o.param_groups:
        n = g["name"]
        p = getattr(m, ATTRS[n])
        assert p is g["params"][0] is out[n] and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.shape[0] == K
        assert torch.equal(p.detach(), old_p[n][keep]) and p.is_contiguous()
        assert torch.equal(o.state[n]["exp_avg"], old_s[n]["exp_avg"][keep]) and torch.equal(o.state[n]["exp_avg_sq"], old_s[n]["exp_avg_sq"][keep])
    assert torch.equal(o.row_mask.bool(), mask[keep])
    # append: cat_tensors_to_optimizer: zeros_like(extension) for both moments, Parameter(cat)
    gen = torch.Generator().manual_seed(4)
    ext = {n: torch.randn((7,) + tuple(getattr(m, ATTRS[n]).shape[1:]), generator=gen) for n in NAMES}
    mid_p = {n: getattr(m, ATTRS[n]).detach().clone() for n in NAMES}
    mid_s = {n: {k: v.clone() for k, v in o.state[n].items()} for n in NAMES}
    out = o.append(ext)
    for g in o.param_groups:
        n = g["name"]
        p = getattr(m, ATTRS[n])
        assert p is g["params"][0] is out[n] and p.shape[0] == K + 7
        assert torch.equal(p.detach(), torch.cat((mid_p[n], ext[n])))
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(o.state[n][k][:K], mid_s[n][k]) and not o.state[n][k][K:].any()
    assert torch.equal(o.row_mask.bool(), torch.cat((mask[keep], torch.ones(7, dtype=torch.bool))))
    before = {n: getattr(m, ATTRS[n]).detach().clone() for n in NAMES}
    set_grads(m, {n: torch.ones_like(before[n]) for n in NAMES})
    o.step()
    live = o.row_mask.bool()
    for n in NAMES:
        p = getattr(m, ATTRS[n]).detach()
        assert (p[live] != before[n][live]).all() and torch.equal(p[~live], before[n][~live]) and live[K:].all()
    # replace: replace_tensor_to_optimizer: both moments zero, Parameter(tensor)
    new_op = torch.full((K + 7, 1), -2.0)
    ret = o.replace("opacity", new_op)
    assert ret is m._opacity is o.param_groups[3]["params"][0] and torch.equal(m._opacity.detach(), new_op)
    assert not o.state["opacity"]["exp_avg"].any() and not o.state["opacity"]["exp_avg_sq"].any()
    assert o.state["xyz"]["exp_avg"].any()
    with pytest.raises(ValueError):
        o.replace("opacity", torch.zeros(3, 1))
    with pytest.raises(ValueError):
        o.append({"xyz": torch.zeros(1, 3)})


def test_a_row_range_follows_prune_and_append():
    m = _stepped_model(rows=(100, 200))
    o = m.optimizer
    assert not o.state["xyz"]["exp_avg"][:100].any() and not o.state["xyz"]["exp_avg"][200:].any() and o.state["xyz"]["exp_avg"][100:200].all()
    keep = torch.ones(P, dtype=torch.bool)
    keep[50:120] = False
    keep[190:210] = False
    o.prune(keep)
    assert o.rows == (50, 120) and o.state["xyz"]["exp_avg"][50:120].all() and not o.state["xyz"]["exp_avg"][120:].any()
    o.append({n: torch.zeros((5,) + tuple(getattr(m, ATTRS[n]).shape[1:])) for n in NAMES})          # appended rows move
    assert o.rows is None and torch.equal(o.row_mask.nonzero().reshape(-1), torch.cat((torch.arange(50, 120), torch.arange(210, 215))))
    tail = _stepped_model(rows=(250, 300)).optimizer
    tail.append({n: torch.zeros((5,) + tuple(getattr(tail.model, ATTRS[n]).shape[1:])) for n in NAMES})
    assert tail.rows == (250, 305) and tail.row_mask is None


def test_state_dict_round_trip():
    mask = torch.arange(P) % 2 == 0
    a = _stepped_model(mask=mask)
    a.update_learning_rate(500)
    sd = a.optimizer.state_dict()
    b = make_model(seed=11)
    for n in NAMES:
        getattr(b, ATTRS[n]).data.copy_(getattr(a, ATTRS[n]).detach())
    b.training_setup(OptimizationParams())
    b.optimizer.load_state_dict(sd)
    assert b.optimizer.step_count == 3 and b.optimizer.param_groups[0]["lr"] == a.optimizer.param_groups[0]["lr"]
    sd["state"]["xyz"]["exp_avg"].zero_()                          # the dict holds copies, and so does the optimiser
    assert a.optimizer.state["xyz"]["exp_avg"].any() and b.optimizer.state["xyz"]["exp_avg"].any()
    for gs in grads(a, steps=2, seed=17):
        for m in (a, b):
            set_grads(m, gs)
            m.optimizer.step()
            m.optimizer.zero_grad()
    for n in NAMES:
        assert torch.equal(getattr(a, ATTRS[n]), getattr(b, ATTRS[n])), n
        assert torch.equal(a.optimizer.state[n]["exp_avg_sq"], b.optimizer.state[n]["exp_avg_sq"])
    with pytest.raises(ValueError):
        GaussianAdam(b, [dict(name="xyz", lr=0.1)]).load_state_dict(sd)


def test_inpaint_setup_with_opt_moves_only_the_tail():
    m = make_model(seed=21)
    removed = torch.zeros(P, dtype=torch.bool)
    removed[40:70] = True
    new = m.inpaint_setup(removed, k=5, opt=OptimizationParams())
    assert int(new.sum()) == 30 and new[-30:].all() and m._xyz.shape[0] == P
    assert isinstance(m.optimizer, GaussianAdam) and m.optimizer.rows == (P - 30, P) and m.optimizer.row_mask is None
    start = {n: getattr(m, ATTRS[n]).detach().clone() for n in NAMES}
    for gs in grads(m, steps=3, seed=23):
        set_grads(m, gs)
        m.optimizer.step()
        m.optimizer.zero_grad()
    for n in NAMES:
        p = getattr(m, ATTRS[n]).detach()
        assert torch.equal(p[:P - 30], start[n][:P - 30]) and (p[P - 30:] != start[n][P - 30:]).all(), n
    m.optimizer.rows = None                                        # the reference's behaviour: every row is trainable
    set_grads(m, grads(m, steps=1, seed=29)[0])
    m.optimizer.step()
    assert (m._xyz.detach()[:P - 30] != start["xyz"][:P - 30]).all()
    # without opt nothing is set up
    m2 = make_model(seed=21)
    m2.inpaint_setup(removed, k=5)
    assert m2.optimizer is None


def test_refusals():
    m = make_model()
    with pytest.raises(ValueError):
        GaussianAdam(m, [dict(name="colour", lr=0.1)])
    with pytest.raises(ValueError):
        GaussianAdam(m, [dict(name="xyz", lr=0.1)], row_mask=torch.ones(P + 1))
    with pytest.raises(ValueError):
        GaussianAdam(m, [dict(name="xyz", lr=0.1)], rows=(5, P + 1))
    with pytest.raises(ValueError):
        m.finetune_setup(OptimizationParams(), torch.ones(P - 1))


def test_create_from_pcd_keeps_the_scale_it_is_given():
    pts = np.random.default_rng(0).standard_normal((50, 3))
    cols = np.random.default_rng(1).uniform(size=(50, 3))
    a = GaussianModel.create_from_pcd(pts, cols, generator=torch.Generator().manual_seed(0))
    b = GaussianModel.create_from_pcd(pts, cols, generator=torch.Generator().manual_seed(0), spatial_lr_scale=4.5)
    assert a.spatial_lr_scale == 1.0 and b.spatial_lr_scale == 4.5
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))

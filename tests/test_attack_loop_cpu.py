"""The order of events of pgd_attack's loop, on the CPU.  The raster path has no CPU form, so attack.render (through which
render_combined renders too) is replaced by a tiny differentiable stand-in: a [3,8,8] image that is a smooth function of
the model's six parameters and a per-camera constant.  Everything is checked against the same loop written out in plain
PyTorch below (as tests/test_gpu_attack.py checks accumulate_grads), never against numbers recorded from the loop itself.

Tolerances: the written-out loop runs the same float32 operations up to their formulation (x - a*g/|g| against an in-place
add of a pre-divided step, the renorm); every step is about ten operations of at most half an ulp (6e-8 relative) each on
values of order one, over at most four iterations: rtol 1e-5 / atol 1e-6 leaves a factor of a few."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from gsplat_attack import attack as A
from gsplat_attack import dist as gdist
from gsplat_attack.scenes import make_scene

ATTRS = {"color": ("_features_rest", "_features_dc"), "position": ("_xyz",), "scaling": ("_scaling",),
         "rotation": ("_rotation",), "opacity": ("_opacity",)}
CLOSE = dict(rtol=1e-5, atol=1e-6)


def _image(model, k: int) -> torch.Tensor:
    """View k's stand-in render: [3,8,8], smooth in all six parameters, different for every Gaussian and every view."""
    P = model._xyz.shape[0]
    w = torch.linspace(-1.0, 1.0, P)[:, None]
    colour = (model._features_dc[:, 0] * w).mean(0) + (model._features_rest.mean(1) * w * w).mean(0)
    geom = ((torch.tanh(model._xyz) * w).mean() + (model._scaling * w).mean() + 0.1 * (model._rotation ** 2).mean()
            + torch.sigmoid(model._opacity * w).mean())
    grid = torch.linspace(0.0, 1.0, 64).reshape(8, 8)
    return torch.sigmoid(colour[:, None, None] * (1 + k) + grid[None] * (geom + 0.1 * k) + 0.05 * k)


def _sum_loss(imgs):
    return (imgs ** 2).mean(dim=(1, 2, 3)).sum()


def _mean_loss(imgs):
    return (imgs ** 2).mean()


def _scene(n_views=3):
    model, cams, _ = make_scene("hydrant-1k", P=50, n_views=n_views)
    return model, cams


def _patch(monkeypatch_or_none, cams, events=None):
    """attack.render -> the stand-in; what a CPU plan must not choose (batch, ring, side stream) raises when touched, and
    the pipe every render is given carries no bucket, no norms and no render cache."""
    def fake_render(cam, model, pipe, bg, *a, **kw):
        k = next(i for i, c in enumerate(cams) if c is cam)
        assert getattr(pipe, "grad_bucket", None) is None and getattr(pipe, "grad_norms", None) is None
        assert getattr(pipe, "render_cache", None) is None
        if events is not None:
            events.append(("render", k, torch.is_grad_enabled()))
        return {"render": _image(model, k)}

    def never(*a, **kw):
        raise AssertionError("the CPU plan chose a device-only path")
    patches = {"render": fake_render, "render_batch": never, "StreamRing": never, "_check_stream": never}
    for name, fn in patches.items():
        if monkeypatch_or_none is None:
            setattr(A, name, fn)
        else:
            monkeypatch_or_none.setattr(A, name, fn)


def _written_out(model, n_views, iters, groups, norm, alpha, eps, stacked, reduction, accumulate):
    """The loop in plain PyTorch -> (history, the parameters after every step)."""
    loss_fn = _mean_loss if reduction == "mean" else _sum_loss
    names = [a for g in groups for a in ATTRS[g]]
    x0 = {a: getattr(model, a).detach().clone() for a in names}
    history, snaps = [], []
    for _ in range(iters):
        if not accumulate:
            for a in gdist.ATTACK_PARAMS:
                getattr(model, a).grad = None
        if stacked:
            loss = loss_fn(torch.stack([_image(model, k) for k in range(n_views)]))     # mean: weight n_views / n_views
            loss.backward()
            total = loss.detach()
        else:
            total = torch.zeros(())
            for k in range(n_views):
                loss = loss_fn(_image(model, k)[None])
                if reduction == "mean":
                    loss = loss / n_views
                loss.backward()
                total = total + loss.detach()
        with torch.no_grad():
            for a in names:
                x, g = getattr(model, a), getattr(model, a).grad
                if norm == "linf":
                    x.copy_(x0[a] + (x - alpha * torch.sign(g) - x0[a]).clamp(-eps, eps))
                else:
                    n = g.norm()
                    d = (x - alpha * g / n if n > 0 else x) - x0[a]
                    rows = d.reshape(d.shape[0], -1).norm(dim=1).reshape(-1, *([1] * (d.dim() - 1)))
                    x.copy_(x0[a] + torch.where(rows > eps, d * (eps / rows), d))
        history.append(float(total))
        snaps.append({a: getattr(model, a).detach().clone() for a in gdist.ATTACK_PARAMS})
    return history, snaps


@pytest.mark.parametrize("groups", [("color",), ("color", "position")])
@pytest.mark.parametrize("norm", ["l2", "linf"])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("stacked", [False, True])
def test_the_loop_equals_the_written_out_loop(monkeypatch, stacked, reduction, accumulate, norm, groups):
    alpha, eps = (0.05, 0.01) if norm == "l2" else (0.05, 0.08)          # the projection engages from the second step on
    model, cams = _scene()
    ref_model, _ = _scene()
    _patch(monkeypatch, cams)
    hist = A.pgd_attack(model, cams, iters=4, alpha=alpha, epsilon=eps, groups=groups, norm=norm, batch_loss=stacked,
                        loss_fn=_mean_loss if reduction == "mean" else _sum_loss, loss_reduction=reduction,
                        accumulate_grads=accumulate)
    want, snaps = _written_out(ref_model, 3, 4, groups, norm, alpha, eps, stacked, reduction, accumulate)
    assert hist == pytest.approx(want, rel=1e-5)
    stepped = {a for g in groups for a in ATTRS[g]}
    for a in gdist.ATTACK_PARAMS:
        torch.testing.assert_close(getattr(model, a).detach(), snaps[-1][a], **CLOSE)
        if a in stepped:
            assert not torch.equal(snaps[-1][a], snaps[0][a]), f"{a} did not move"


@pytest.mark.parametrize("stacked", [False, True])
def test_a_loss_with_takes_view_index_receives_the_global_indices(monkeypatch, stacked):
    model, cams = _scene()
    _patch(monkeypatch, cams)
    seen = []

    def loss_fn(imgs, idx=None):
        seen.append((tuple(imgs.shape), list(idx)))
        return _sum_loss(imgs)
    loss_fn.takes_view_index = True
    A.pgd_attack(model, cams, iters=2, loss_fn=loss_fn, batch_loss=stacked)
    one = [((3, 3, 8, 8), [0, 1, 2])] if stacked else [((1, 3, 8, 8), [k]) for k in range(3)]
    assert seen == one * 2


def _scheduled(table, n_views, model, calls):
    """success_fn whose answer for (iteration, view) is table[iteration][view]; every call is recorded with the colour
    parameters it saw."""
    def success_fn(image, view):
        it = len(calls) // n_views
        calls.append((it, view, model._features_dc.detach().clone(), image.detach().clone()))
        return table[min(it, len(table) - 1)][view]
    return success_fn


@pytest.mark.parametrize("n_views,table,stop_at", [(3, [[False] * 3, [True, False, False], [True, False, True]], 2),
                                                   (3, [[False] * 3], None),
                                                   (1, [[False], [True]], 1)])      # B - 1 = 0 would stop a lone view at once
@pytest.mark.parametrize("save", [False, True])
def test_success_check_order_stop_and_save(monkeypatch, n_views, table, stop_at, save):
    model, cams = _scene(n_views)
    ref_model, _ = _scene(n_views)
    events, calls, recs, saved = [], [], [], []
    _patch(monkeypatch, cams, events)
    monkeypatch.setattr(model, "save_ply", saved.append, raising=False)
    iters = 5
    hist = A.pgd_attack(model, cams, iters=iters, alpha=0.05, epsilon=0.01, loss_fn=_sum_loss, log=recs.append,
                        success_fn=_scheduled(table, n_views, model, calls), save_path="out.ply" if save else None)
    ran = iters if stop_at is None else stop_at + 1
    _, snaps = _written_out(ref_model, n_views, ran, ("color",), "l2", 0.05, 0.01, False, "sum", False)
    assert len(hist) == ran and [r["iter"] for r in recs] == list(range(ran))
    # once per view and iteration, in view order, on the parameters that iteration's step left and on their render
    assert [(it, v) for it, v, _, _ in calls] == [(it, v) for it in range(ran) for v in range(n_views)]
    for it, v, dc, image in calls:
        torch.testing.assert_close(dc, snaps[it]["_features_dc"], **CLOSE)
    torch.testing.assert_close(calls[-1][3], _image(ref_model, n_views - 1).detach(), **CLOSE)      # ref_model is at snaps[-1]
    # per iteration: the views' forwards with gradient, then (behind the step) their success renders without
    per_it = [("render", k, True) for k in range(n_views)] + [("render", k, False) for k in range(n_views)]
    assert events == per_it * ran
    want_flags = [list(table[min(it, len(table) - 1)]) for it in range(ran)]
    assert [r["successes"] for r in recs] == want_flags and A.pgd_attack.last_successes == want_flags[-1]
    assert all(set(r) == {"iter", "loss", "views", "successes", "seconds"} and r["views"] == n_views for r in recs)
    assert [r["loss"] for r in recs] == hist
    assert saved == (["out.ply"] if save and stop_at is not None else [])


def test_log_records_without_a_success_check(monkeypatch):
    model, cams = _scene()
    _patch(monkeypatch, cams)
    recs = []
    hist = A.pgd_attack(model, cams, iters=3, loss_fn=_sum_loss, log=recs.append)
    assert len(hist) == 3 and A.pgd_attack.last_successes is None
    assert all(set(r) == {"iter", "loss", "views", "seconds"} for r in recs) and [r["loss"] for r in recs] == hist


def test_a_timer_sees_every_phase_of_the_per_view_loop(monkeypatch):
    """Any object with start() / lap(phase) serves as the timer: the per-view form's sequence of phases."""
    model, cams = _scene()
    _patch(monkeypatch, cams)

    class Laps:
        def __init__(self):
            self.seen = []

        def start(self):
            self.seen.append("start")

        def lap(self, phase):
            self.seen.append(phase)
    laps = Laps()
    A.pgd_attack(model, cams, iters=2, loss_fn=_sum_loss, timer=laps, success_fn=lambda im, i: False)
    assert laps.seen == (["start"] + ["render", "loss", "backward"] * 3 + ["reduce", "step", "rerender"]) * 2
    assert set(laps.seen) - {"start"} == set(A.PhaseTimer.PHASES)


def test_frozen_geometry_is_unfrozen_on_every_exit(monkeypatch):
    model, cams = _scene()
    _patch(monkeypatch, cams)
    seen = []

    def loss_fn(imgs):
        seen.append([getattr(model, a).requires_grad for a in gdist.ATTACK_PARAMS])
        return _sum_loss(imgs)
    A.pgd_attack(model, cams, iters=1, groups=("color",), loss_fn=loss_fn)
    geometry = [a not in ("_features_dc", "_features_rest") for a in gdist.ATTACK_PARAMS]
    assert seen and all(s == [not g for g in geometry] for s in seen)        # frozen while the attack runs
    assert all(getattr(model, a).requires_grad for a in gdist.ATTACK_PARAMS)

    def raising(imgs):
        raise RuntimeError("the detector failed")
    with pytest.raises(RuntimeError, match="the detector failed"):
        A.pgd_attack(model, cams, iters=1, groups=("color",), loss_fn=raising)
    assert all(getattr(model, a).requires_grad for a in gdist.ATTACK_PARAMS)


# ---- two gloo ranks ----------------------------------------------------------------------------------------------------

RANK_CASES = [dict(accumulate_grads=False), dict(accumulate_grads=True),
              dict(batch_loss=True, loss_reduction="mean", loss_fn=_mean_loss)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _attack_case(n_views, case):
    """One case on this process's rank (or alone) -> what the ranks and the single process are compared on."""
    model, cams = _scene(n_views)
    _patch(None, cams)
    seen, ids = {}, []

    def success_fn(image, view):                   # view 0 succeeds from its second check on
        seen[view] = seen.get(view, 0) + 1
        return view == 0 and seen[view] >= 2
    base = case.get("loss_fn", _sum_loss)

    def loss_fn(imgs, idx=None):
        ids.append(list(idx))
        return base(imgs)
    loss_fn.takes_view_index = True
    kw = {k: v for k, v in case.items() if k != "loss_fn"}
    hist = A.pgd_attack(model, cams, iters=2, alpha=0.05, epsilon=0.01, groups=("color", "position"), loss_fn=loss_fn,
                        success_fn=success_fn, **kw)
    out = {a: getattr(model, a).detach().clone() for a in gdist.ATTACK_PARAMS}
    out.update({"grad" + a: getattr(model, a).grad for a in ("_features_dc", "_features_rest", "_xyz")})
    out.update(history=hist, flags=A.pgd_attack.last_successes, ids=ids)
    return out


def _rank_worker(rank, world, port, n_views, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    gdist.init_from_env("gloo")
    torch.save([_attack_case(n_views, case) for case in RANK_CASES], os.path.join(out_dir, f"r{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("n_views", [3, 1])            # one view: rank 1 has none
def test_two_gloo_ranks_equal_the_single_process(tmp_path, monkeypatch, n_views):
    world, port = 2, _free_port()
    mp.spawn(_rank_worker, args=(world, port, n_views, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for name in ("render", "render_batch", "StreamRing", "_check_stream"):
        monkeypatch.setattr(A, name, getattr(A, name))                   # _patch(None, ...) below is undone afterwards
    for case, a, b in zip(RANK_CASES, r0, r1):
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert torch.equal(a[k], b[k]), f"replicas diverged on {k} ({case})"
        assert a["history"] == b["history"] and a["flags"] == b["flags"] == [True, False, False][:n_views]
        stacked = bool(case.get("batch_loss"))
        mine = lambda r: [v for v in range(n_views) if v % world == r]
        for r, got in ((0, a), (1, b)):
            one = ([mine(r)] if mine(r) else []) if stacked else [[v] for v in mine(r)]
            assert got["ids"] == one * 2
        alone = _attack_case(n_views, case)
        assert a["history"] == pytest.approx(alone["history"], rel=1e-6)
        # the same loop written out: with accumulate_grads its second step uses the sum of both (reduced) gradients
        ref_model, _ = _scene(n_views)
        _, snaps = _written_out(ref_model, n_views, 2, ("color", "position"), "l2", 0.05, 0.01, stacked,
                                case.get("loss_reduction", "sum"), bool(case.get("accumulate_grads")))
        for n in gdist.ATTACK_PARAMS:
            torch.testing.assert_close(a[n], snaps[-1][n], **CLOSE)
            torch.testing.assert_close(a[n], alone[n], **CLOSE)
        for n in ("grad_features_dc", "grad_features_rest", "grad_xyz"):
            torch.testing.assert_close(a[n], getattr(ref_model, n[4:]).grad, **CLOSE)

"""finetune_setup + refit end to end on the device: scene hydrant-1k at 128 x 128, two cameras, the colours of a masked tenth of
the Gaussians perturbed, 30 steps against the unperturbed renders.  A direction and repeatability check: the loss falls, the
rows outside the mask keep their bits, two runs agree bit for bit.  No particular final loss is asserted."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ITERS = 30


def _run():
    from gsplat_attack.optim import OptimizationParams, refit
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device="cuda", n_views=2, width=128, height=128)
    P = model._xyz.shape[0]
    bg = torch.zeros(3, device="cuda")
    pipe = PipelineParams(skip_objects=True)
    with torch.no_grad():
        targets = torch.stack([render(c, model, pipe, bg)["render"] for c in cams]).clone()
    mask = torch.zeros(P, dtype=torch.bool, device="cuda")
    mask[torch.randperm(P, generator=torch.Generator().manual_seed(3))[:P // 10].cuda()] = True
    with torch.no_grad():
        noise = torch.randn(P, 1, 3, generator=torch.Generator().manual_seed(4)).cuda()
        model._features_dc[mask] += 0.8 * noise[mask]
    start = [p.detach().clone() for p in model.parameters()]
    model.finetune_setup(OptimizationParams(), mask[:, None].float())
    losses = refit(model, cams, targets, iters=ITERS, pipe=pipe, background=bg)
    torch.cuda.synchronize()
    return model, mask, start, losses.cpu()


def test_refit_lowers_the_loss_leaves_unmasked_rows_alone_and_repeats_bit_for_bit():
    model, mask, start, losses = _run()
    assert losses.shape == (ITERS,) and torch.isfinite(losses).all()
    first, last = losses[:2].mean().item(), losses[-2:].mean().item()        # (two cameras in turn: compare like with like)
    print(f"refit: loss {first:.5f} -> {last:.5f}")
    assert losses[-1] < losses[0]
    assert losses[-2] < losses[0] and losses[-1] < losses[1] and last < first
    assert model.optimizer.step_count == ITERS
    moved = 0
    for name, p, s in zip(model.named_parameters(), model.parameters(), start):
        assert torch.equal(p.detach()[~mask], s[~mask]), name                 # bit for bit
        moved += int((p.detach()[mask] != s[mask]).any())
    assert moved >= 6 and torch.equal(model._objects_dc, start[6])            # the frozen group
    model2, _, _, losses2 = _run()
    assert torch.equal(losses, losses2)
    for p, q in zip(model.parameters(), model2.parameters()):
        assert torch.equal(p, q)

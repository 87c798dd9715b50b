"""The detector loss stage on the device: every case of tests/detloss_cases.py against the float64 PyTorch oracle (tgt
integer-equal; ts, loss[4] and grad_pred within 4 x the float32 oracle's own error, floor 2^-22, never above 1e-3), the same
bits on every call, on a side stream and without grad_pred, and the stage behind a small torch head as pgd_attack's loss_fn:
render -> letterbox -> head -> loss -> backward to the Gaussian parameters, bit for bit repeatable."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detloss_cases as DC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def LO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import detloss_ops
    D._load()
    assert detloss_ops.available()
    return detloss_ops


def _dev(ref):
    return (torch.tensor(np.array(ref["pred"])).to(DEV), torch.tensor(np.array(ref["gt_boxes"])).to(DEV),
            torch.tensor(np.array(ref["gt_cls"])).to(DEV))


def _check(c, got, ref, who):
    """tgt integer-equal, ts / loss / grad within the bound; prints each figure first."""
    o = ref["o64"]
    assert torch.equal(got["tgt"].cpu(), o["tgt"]), f"{who} {c.id}: tgt differs"
    fails = []
    for k in DC.COMPARED:
        e, y = DC.err(got[k], o[k]), ref["yard"][k]
        b = DC.bound(y)
        print(f"{who} {c.id} {k}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {b:.3e}")
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, f"{who} {c.id}: {fails}"


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("c", DC.CASES, ids=lambda c: c.id)
def test_kernels_against_the_oracle_and_repeat(LO, c):
    ref = DC.reference(c)
    assert DC.margins_ok(ref["o64"])
    pred, gtb, gtc = _dev(ref)
    loss, grad, tgt, ts = LO.run(pred, c.levels, gtb, gtc)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
    _check(c, dict(tgt=tgt, ts=ts, loss=loss, grad=grad), ref, "device")
    # background anchors: zeros in their 64 box channels
    assert (grad[:, :64].permute(0, 2, 1)[tgt < 0] == 0).all()
    # the same call again, and once on a side stream: identical bits
    again = LO.run(pred, c.levels, gtb, gtc)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = LO.run(pred, c.levels, gtb, gtc)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b2, b3 in zip((loss, grad, tgt, ts), again, other):
        assert _bits(a) == _bits(b2) and _bits(a) == _bits(b3)
    # grad_pred = NULL and no tgt / ts outputs: the same loss bits
    bare = LO.run(pred, c.levels, gtb, gtc, want_grad=False, want_assignment=False)
    assert bare[1] is None and bare[2] is None and _bits(bare[0]) == _bits(loss)


def test_unaligned_pred_takes_the_scalar_path(LO):
    """A % 4 == 0 but pred starts 4 bytes past a 16-byte boundary: one anchor per lane.  The assignment and every gradient
    element are the same bits; the loss sums run over other tiles, so it is compared with the oracle."""
    c = DC.BY_ID["tiny"]
    ref = DC.reference(c)
    pred, gtb, gtc = _dev(ref)
    base = LO.run(pred, c.levels, gtb, gtc)
    store = torch.empty(pred.numel() + 1, dtype=torch.float32, device=DEV)
    shifted = store[1:].view(pred.shape)
    shifted.copy_(pred)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    loss, grad, tgt, ts = LO.run(shifted, c.levels, gtb, gtc)
    torch.cuda.synchronize()
    assert _bits(grad) == _bits(base[1]) and _bits(tgt) == _bits(base[2]) and _bits(ts) == _bits(base[3])
    _check(c, dict(tgt=tgt, ts=ts, loss=loss, grad=grad), ref, "scalar path")


def test_autograd_function(LO):
    c = DC.BY_ID["ragged"]
    ref = DC.reference(c)
    pred, gtb, gtc = _dev(ref)
    x = pred.clone().requires_grad_(True)
    total, items = LO.detloss(x, c.levels, gtb, gtc)
    assert not items.requires_grad and total.requires_grad
    (total * 3.0).backward()
    loss, grad, _, _ = LO.run(pred, c.levels, gtb, gtc)
    assert _bits(total) == _bits(loss[3]) and _bits(items) == _bits(loss[:3])
    assert torch.equal(x.grad, grad * 3.0)
    with torch.no_grad():
        t2, _ = LO.detloss(pred, c.levels, gtb, gtc)
    assert _bits(t2) == _bits(loss[3])


# ---- end to end -------------------------------------------------------------------------------------------------------------
NC, NET = 3, 96            # classes of the head; the letterboxed input is NET x NET
STRIDES = (8, 16, 32)
GT = torch.tensor([[10.3, 12.6, 52.2, 49.7], [14.4, 7.7, 56.3, 54.1], [8.9, 14.2, 50.6, 55.8]])   # per view, render frame
TARGET = 1


class Head(torch.nn.Module):
    """Three strided convolutions of the network input -> [B, 64 + NC, h_i, w_i]; fixed-seed weights, a bias that makes every
    side's bins peak near 3 cells so that the predicted boxes overlap the gt box."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(21)
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(3, 64 + NC, s, stride=s) for s in STRIDES)
        k = torch.arange(16, dtype=torch.float32)
        with torch.no_grad():
            for conv, s in zip(self.convs, STRIDES):
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (0.8 / s))
                conv.bias[:64] = (-0.5 * ((k - 24.0 / s) / 1.2) ** 2).repeat(4)
                conv.bias[64:] = torch.randn(NC, generator=g)

    def forward(self, x):
        return [conv(x) for conv in self.convs]


def _scene():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), width=64, height=64, n_views=3)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _loss_fn():
    from gsplat_attack.detector_input import DetectorInput, letterbox_geometry
    from gsplat_attack.detector_loss import DetectorLoss, make_loss_fn
    scale, _, _, top, left = letterbox_geometry(64, 64, (NET, NET))
    head = Head().to(DEV)
    dl = DetectorLoss(NC, STRIDES).to_letterbox(scale, left, top)
    return make_loss_fn(head, DetectorInput(letterbox=(NET, NET)), dl, GT, TARGET), head, (scale, left, top)


def test_loss_fn_gradients_reach_the_gaussians_and_repeat():
    from gsplat_attack.renderer import PipelineParams, render_batch
    model, cams, bg = _scene()
    loss_fn, _, _ = _loss_fn()
    raw = [model.named_parameters()[n] for n in ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")]
    runs = []
    for _ in range(2):
        model.zero_grad()
        renders = render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"]
        total = loss_fn(renders, idx=[0, 1, 2])
        total.backward()
        runs.append([total.detach().clone()] + [p.grad.detach().clone() for p in raw])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0
        assert torch.equal(a, b)


def test_pgd_attack_with_the_detection_loss_repeats():
    from gsplat_attack.attack import pgd_attack
    hists = []
    for batch_loss in (True, True, False, False):
        model, cams, bg = _scene()
        loss_fn, _, _ = _loss_fn()
        hists.append(pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=batch_loss, loss_fn=loss_fn))
    for h in hists:
        assert len(h) == 2 and all(np.isfinite(v) for v in h) and h[0] != h[1]     # the step moved the loss
    assert hists[0] == hists[1] and hists[2] == hists[3]


def test_gradient_to_the_renders_against_the_oracle_behind_the_same_head():
    """d total / d renders: HIP letterbox -> head on the device -> HIP loss, against F.interpolate + F.pad -> the same head
    -> the oracle, in float64 on the CPU; the yardstick is that CPU chain in float32."""
    from gsplat_attack.detector_input import GREY
    from gsplat_attack.renderer import PipelineParams, render_batch
    model, cams, bg = _scene()
    loss_fn, head, (scale, left, top) = _loss_fn()
    with torch.no_grad():
        renders = render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"].detach().clone()
    x = renders.clone().requires_grad_(True)
    total = loss_fn(x, idx=[0, 1, 2])
    total.backward()
    torch.cuda.synchronize()

    def chain(dtype):
        h = Head().to(dtype)
        r = renders.cpu().to(dtype).requires_grad_(True)
        rs = int(round(64 * scale))
        img = F.pad(F.interpolate(r, size=(rs, rs), mode="bilinear", align_corners=False),
                    (left, NET - rs - left, top, NET - rs - top), value=GREY)
        feats = h(img)
        levels = [(int(f.shape[2]), int(f.shape[3]), float(s)) for f, s in zip(feats, STRIDES)]
        pred = torch.cat([f.reshape(f.shape[0], f.shape[1], -1) for f in feats], dim=2)
        gt = (GT.to(dtype) * scale + torch.tensor([left, top, left, top], dtype=dtype))[:, None, :]
        o = DC.oracle(levels, pred, gt, torch.full((3, 1), TARGET), dtype)
        o["total"].backward()
        return o, r.grad.detach()

    o64, g64 = chain(torch.float64)
    o32, g32 = chain(torch.float32)
    print(f"end to end: gaps topk {o64['gap_topk']:.3e} candidate {o64['gap_candidate']:.3e} conflict {o64['gap_conflict']:.3e} "
          f"dfl {o64['gap_dfl']:.3e} fg {int((o64['tgt'] >= 0).sum())}")
    assert DC.margins_ok(o64) and torch.equal(o32["tgt"], o64["tgt"]) and (o64["tgt"] >= 0).any()
    for name, got, want, yard in (("total", total.detach(), o64["total"].detach(), o32["total"].detach()),
                                  ("d total / d renders", x.grad, g64, g32)):
        e, y = DC.err(got, want), DC.err(yard, want)
        print(f"end to end {name}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {DC.bound(y):.3e}")
        assert e <= DC.bound(y), name

"""The detector loss stage on the device: every case of tests/detloss_cases.py, with the case's own spec and level table,
against the float64 PyTorch oracle (tgt integer-equal; ts, loss[4] and grad_pred within 4 x the float32 oracle's own error,
floor 2^-22, never above 1e-3), the same bits on every call, on a side stream and without grad_pred; the entry point itself
on outputs and a workspace that lie between guards (nothing written outside, every element written, prior workspace contents
without effect); pred or grad_pred off a 16-byte boundary against the aligned call; DetectorLoss on device tensors; and the
stage behind a small torch head as pgd_attack's loss_fn: render -> letterbox -> head -> loss -> backward to the Gaussian
parameters, bit for bit repeatable.  DESIGN.md's table has the measured ratios."""
import ctypes

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


def _spec(LO, c):
    return LO.DetLossSpec(c.topk, c.alpha, c.beta, *c.w)


@pytest.mark.parametrize("c", DC.CASES, ids=lambda c: c.id)
def test_kernels_against_the_oracle_and_repeat(LO, c):
    ref = DC.reference(c)
    assert DC.margins_ok(ref["o64"]) and ref["yard_tgt_equal"]
    pred, gtb, gtc = _dev(ref)
    spec = _spec(LO, c)
    loss, grad, tgt, ts = LO.run(pred, c.levels, gtb, gtc, spec)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and torch.isfinite(loss).all()
    _check(c, dict(tgt=tgt, ts=ts, loss=loss, grad=grad), ref, "device")
    # background anchors: zeros in their 64 box channels
    assert (grad[:, :64].permute(0, 2, 1)[tgt < 0] == 0).all()
    if c.id == "collapsed":                                   # the two tie rules by hand, not through the oracle
        assert np.array_equal(tgt[0].cpu().numpy(), DC.tie_rules_by_hand(c, ref["gt_boxes"], ref["gt_cls"], 0)[1])
        assert (ts[0] == 0).all() and (ts[1] > 0).any()
    if c.id == "all-absent":
        assert (tgt == -1).all() and (ts == 0).all() and loss[0] == 0 and loss[2] == 0 and (grad[:, :64] == 0).all()
    if c.id == "weights":
        assert (grad[:, 64:] == 0).all() and (grad[:, :64] != 0).any()
    if c.id == "cls-only":
        assert (grad[:, :64] == 0).all() and (grad[:, 64:] != 0).any()
    # the same call again, and once on a side stream: identical bits
    again = LO.run(pred, c.levels, gtb, gtc, spec)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = LO.run(pred, c.levels, gtb, gtc, spec)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b2, b3 in zip((loss, grad, tgt, ts), again, other):
        assert _bits(a) == _bits(b2) and _bits(a) == _bits(b3)
    # grad_pred = NULL and no tgt / ts outputs: the same loss bits
    bare = LO.run(pred, c.levels, gtb, gtc, spec, want_grad=False, want_assignment=False)
    assert bare[1] is None and bare[2] is None and _bits(bare[0]) == _bits(loss)


# ---- the entry point itself, on buffers between guards ------------------------------------------------------------------------
GUARD = 64                 # elements on either side of an output; 256 bytes, so that a view behind it keeps its alignment
PATTERN = 0x5A5A5A5A       # the guards' bit pattern
WS_GUARD = 256             # bytes behind the workspace


class _Guarded:
    """n 4-byte elements between two guards, `shift` elements past a 16-byte boundary; pre-filled with NaN or -9."""

    def __init__(self, n, dtype, shift=0):
        self.store = torch.full((GUARD + shift + n + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.view = self.store[self.lo:self.hi].view(dtype)
        self.view.fill_(float("nan") if dtype == torch.float32 else -9)
        assert self.view.data_ptr() % 16 == 4 * shift

    def intact(self):
        return bool((self.store[:self.lo] == PATTERN).all() and (self.store[self.hi:] == PATTERN).all())


def _raw(LO, c, ref, ws_fill, grad_shift=0):
    """gsr_detloss called directly: grad_pred, tgt, ts and loss are views of larger buffers, the workspace has exactly
    gsr_detloss_workspace_bytes bytes of ws_fill and a guard behind it -> dict(loss, grad, tgt, ts), guards checked."""
    from diff_gaussian_rasterization import _ops_common
    pred, gtb, gtc = _dev(ref)
    assert pred.data_ptr() % 16 == 0
    cs = LO.c_spec(_spec(LO, c), c.levels, c.B, c.C, c.M)
    nbytes = LO.workspace_bytes(cs)
    wstore = torch.full((nbytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    wstore[:nbytes] = ws_fill
    assert wstore.data_ptr() % 16 == 0
    n = c.B * c.A
    bufs = dict(loss=_Guarded(4, torch.float32), grad=_Guarded(pred.numel(), torch.float32, grad_shift),
                tgt=_Guarded(n, torch.int32), ts=_Guarded(n, torch.float32))
    _ops_common.call("gsr_detloss", pred.device, ctypes.byref(cs), pred.data_ptr(), gtb.data_ptr(), gtc.data_ptr(), wstore.data_ptr(),
                     nbytes, bufs["loss"].view.data_ptr(), bufs["grad"].view.data_ptr(), bufs["tgt"].view.data_ptr(),
                     bufs["ts"].view.data_ptr())
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert g.intact(), f"{c.id}: a store outside {k}"
    assert (wstore[nbytes:] == 0xA5).all(), f"{c.id}: a store behind the workspace"
    out = dict(loss=bufs["loss"].view.clone(), grad=bufs["grad"].view.clone().view(pred.shape), tgt=bufs["tgt"].view.clone().view(c.B, c.A),
               ts=bufs["ts"].view.clone().view(c.B, c.A))
    for k in ("loss", "grad", "ts"):
        assert not torch.isnan(out[k]).any(), f"{c.id}: an element of {k} was not written"
    assert (out["tgt"] != -9).all(), f"{c.id}: an element of tgt was not written"
    return out


@pytest.mark.parametrize("cid", ["tiny", "ragged", "straddle", "long-slab", "collapsed", "topk-16-rows-32"])
def test_outputs_and_workspace_between_guards(LO, cid):
    """Nothing is written outside grad_pred, tgt, ts, loss or the workspace; every output element is written; what the
    workspace held before (0xFF bytes: NaNs and -1; zeros) does not matter; the bits are those of detloss_ops.run."""
    c = DC.BY_ID[cid]
    ref = DC.reference(c)
    ones, zeros = _raw(LO, c, ref, 0xFF), _raw(LO, c, ref, 0)
    pred, gtb, gtc = _dev(ref)
    base = LO.run(pred, c.levels, gtb, gtc, _spec(LO, c))
    torch.cuda.synchronize()
    for k, b in zip(("loss", "grad", "tgt", "ts"), base):
        assert _bits(ones[k]) == _bits(zeros[k]) == _bits(b), k


@pytest.mark.parametrize("cid", ["tiny", "straddle"])
def test_unaligned_grad_pred_takes_the_scalar_path(LO, cid):
    """A % 4 == 0 and pred on a 16-byte boundary, but grad_pred starts 4 bytes past one: one anchor per lane.  The assignment
    and every gradient element are the same bits as the aligned call's; the loss sums run over other tiles, so it is
    compared with the oracle."""
    c = DC.BY_ID[cid]
    assert c.A % 4 == 0
    ref = DC.reference(c)
    base, got = _raw(LO, c, ref, 0), _raw(LO, c, ref, 0, grad_shift=1)
    for k in ("grad", "tgt", "ts"):
        assert _bits(got[k]) == _bits(base[k]), k
    _check(c, got, ref, "scalar path (grad_pred)")


def _unaligned_pred(LO, c):
    ref = DC.reference(c)
    pred, gtb, gtc = _dev(ref)
    spec = _spec(LO, c)
    base = LO.run(pred, c.levels, gtb, gtc, spec)
    store = torch.empty(pred.numel() + 1, dtype=torch.float32, device=DEV)
    shifted = store[1:].view(pred.shape)
    shifted.copy_(pred)
    assert c.A % 4 == 0 and pred.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    loss, grad, tgt, ts = LO.run(shifted, c.levels, gtb, gtc, spec)
    torch.cuda.synchronize()
    assert _bits(grad) == _bits(base[1]) and _bits(tgt) == _bits(base[2]) and _bits(ts) == _bits(base[3])
    _check(c, dict(tgt=tgt, ts=ts, loss=loss, grad=grad), ref, "scalar path")


def test_unaligned_pred_takes_the_scalar_path(LO):
    """A % 4 == 0 but pred starts 4 bytes past a 16-byte boundary: one anchor per lane.  The assignment and every gradient
    element are the same bits; the loss sums run over other tiles, so it is compared with the oracle."""
    _unaligned_pred(LO, DC.BY_ID["tiny"])


def test_vector_path_equals_the_scalar_path_across_a_level_boundary(LO):
    """The same on `straddle`, where lanes of the 16-byte path own four anchors of two levels with foreground on both."""
    c = DC.BY_ID["straddle"]
    assert DC.straddling_groups(c, DC.reference(c)["o64"]["tgt"])
    _unaligned_pred(LO, c)


# ---- the Python surface on device tensors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["weights", "few-anchors"])
def test_detector_loss_class_on_the_device(LO, cid):
    """DetectorLoss with a flat pred, input_hw and a non-default spec: .loss() and .assignment() are detloss_ops.run's bits;
    a [B,4] / [B] ground truth with a NaN row is the [B,1,4] form with that row's class -1; .to_letterbox() on render-frame
    boxes is the mapped boxes passed directly."""
    from gsplat_attack.detector_loss import DetectorLoss
    c = DC.BY_ID[cid]
    ref = DC.reference(c)
    pred, gtb, gtc = _dev(ref)
    spec = _spec(LO, c)
    assert spec != LO.DetLossSpec()
    dl = DetectorLoss(c.C, c.strides, input_hw=c.hw, topk=c.topk, alpha=c.alpha, beta=c.beta, box=c.w[0], cls=c.w[1], dfl=c.w[2])
    loss, _, tgt, ts = LO.run(pred, c.levels, gtb, gtc, spec)
    total, items = dl.loss(pred, gtb, gtc)
    a_tgt, a_ts = dl.assignment(pred, gtb, gtc)
    torch.cuda.synchronize()
    assert _bits(total) == _bits(loss[3]) and _bits(items) == _bits(loss[:3])
    assert _bits(a_tgt) == _bits(tgt) and _bits(a_ts) == _bits(ts) and (tgt >= 0).any()
    # one row per image, image 0's a NaN row
    one_b, one_c = gtb[:, 0, :].clone(), gtc[:, 0].clone()
    assert 0 <= one_c[0] < c.C and (tgt[0] == 0).any()
    nan_b = one_b.clone()
    nan_b[0, 2] = float("nan")
    gone_c = one_c.clone()
    gone_c[0] = -1
    want = LO.run(pred, c.levels, one_b[:, None, :], gone_c[:, None], spec)
    got_l, got_a = dl.loss(pred, nan_b, one_c), dl.assignment(pred, nan_b, one_c)
    explicit = dl.loss(pred, one_b[:, None, :], gone_c[:, None])
    torch.cuda.synchronize()
    assert _bits(got_l[0]) == _bits(explicit[0]) == _bits(want[0][3]) and _bits(got_l[1]) == _bits(explicit[1]) == _bits(want[0][:3])
    assert _bits(got_a[0]) == _bits(want[2]) and _bits(got_a[1]) == _bits(want[3]) and (want[2][0] == -1).all()
    # boxes in the render's frame
    s, l, t = 0.75, 4.0, 2.0
    shift = torch.tensor([l, t, l, t], dtype=torch.float32)
    render = (torch.tensor(np.array(ref["gt_boxes"])) - shift) / s
    mapped = render * s + shift                                # what _gt computes, in float32
    lb = dl.to_letterbox(s, l, t)
    got, want = lb.loss(pred, render, gtc), dl.loss(pred, mapped, gtc)
    got_a, want_a = lb.assignment(pred, render.to(DEV), gtc), dl.assignment(pred, mapped, gtc)
    torch.cuda.synchronize()
    assert _bits(got[0]) == _bits(want[0]) and _bits(got[1]) == _bits(want[1])
    assert _bits(got_a[0]) == _bits(want_a[0]) and _bits(got_a[1]) == _bits(want_a[1]) and (want_a[0] >= 0).any()
    assert dl.affine == (1.0, 0.0, 0.0)                        # to_letterbox returns a copy


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

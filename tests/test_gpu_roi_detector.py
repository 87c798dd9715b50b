"""The two-stage detector stage on the device: every case of tests/rcnn_cases.py against the float64 PyTorch oracle (the
sampler's idx, labels, gt_row, counts and the output stage's counts, kept classes and kept order integer-equal to the oracle
and to the host build; pooled, grad_features, loss, grad_scores and grad_deltas within 4 x the float32 oracle's own error,
floor 2^-22, never above 1e-3), the margins asserted in front of every comparison, every output element written, the same
bits on every call and on a side stream, `accumulate`, the autograd functions, verdicts against a host restatement, and
the stage behind a small torch backbone and box head as pgd_attack's loss_fn, bit for bit repeatable."""
import ctypes

import numpy as np
import pytest
import torch

import rcnn_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
ISENT = -777


@pytest.fixture(scope="module")
def RO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import rcnn_ops
    D._load()
    assert rcnn_ops.available()
    return rcnn_ops


@pytest.fixture(scope="module")
def host():
    return RC.host_lib()


def _t(a):
    return None if a is None else torch.tensor(np.array(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(who, cid, got, ref, keys):
    fails = []
    for k in keys:
        e, y = RC.err(got[k], ref["o64"][k]), ref["yard"][k]
        b = RC.bound(y)
        print(f"{who} {cid} {k}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {b:.3e}")
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, f"{who} {cid}: {fails}"


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def _raw_sample(RO, c, seed):
    """The C entry on sentinel-filled caller buffers."""
    prop, gt, cls, n_prop = (_t(a) for a in RC.sample_inputs(c))
    cs = RO.c_spec(RO.RcnnSpec(S=c.S, max_pos=c.max_pos, append_gt=c.append_gt, seed=seed, fg_iou=RC.FG_IOU), B=RC.B, R=c.R, M=c.M, C=RC.NC)
    out = dict(idx=torch.full((RC.B, c.S), ISENT, dtype=torch.int32, device=DEV),
               rois=torch.full((RC.B, c.S, 4), SENTINEL, dtype=torch.float32, device=DEV),
               labels=torch.full((RC.B, c.S), ISENT, dtype=torch.int32, device=DEV),
               gt_row=torch.full((RC.B, c.S), ISENT, dtype=torch.int32, device=DEV),
               counts=torch.full((RC.B, 2), ISENT, dtype=torch.int32, device=DEV))
    lib = RO._lib()
    rc = lib.gsr_rcnn_sample(ctypes.byref(cs), prop.data_ptr(), None if n_prop is None else n_prop.data_ptr(), gt.data_ptr(),
                             cls.data_ptr(), out["idx"].data_ptr(), out["rois"].data_ptr(), out["labels"].data_ptr(),
                             out["gt_row"].data_ptr(), out["counts"].data_ptr(), _stream())
    assert rc == 0, lib.gsr_last_error()
    return out


@pytest.mark.parametrize("c", RC.SAMPLE_CASES, ids=lambda c: c.id)
def test_sampler_equals_the_oracle_and_the_host_build(RO, host, c):
    o, h = RC.sample_reference(c), RC.host_sample(host, c)
    assert RC.sample_margins_ok(o)
    got = _raw_sample(RO, c, c.seed)
    for k in ("idx", "labels", "gt_row", "counts"):
        g = got[k].cpu().numpy()
        assert not (g == ISENT).any(), f"{c.id}: {k} holds unwritten elements"
        assert np.array_equal(g, o[k]) and np.array_equal(g, h[k]), f"{c.id}: {k} differs"
    assert _bits(got["rois"]) == o["rois"].tobytes() == h["rois"].tobytes()
    # the binding, the same seed: the same bits
    prop, gt, cls, n_prop = (_t(a) for a in RC.sample_inputs(c))
    spec = RO.RcnnSpec(S=c.S, max_pos=c.max_pos, append_gt=c.append_gt, seed=c.seed)
    again = RO.sample(prop, gt, cls, RC.NC, spec, n_prop=n_prop)
    for k in ("idx", "rois", "labels", "gt_row", "counts"):
        assert _bits(getattr(again, k)) == _bits(got[k])


def test_sampler_seeds(RO):
    c = RC.SAMPLE_CASES[2]
    a, b = _raw_sample(RO, c, 1), _raw_sample(RO, c, 2)
    assert np.array_equal(a["idx"].cpu().numpy(), RC.sample_reference(c, 1)["idx"])
    assert np.array_equal(b["idx"].cpu().numpy(), RC.sample_reference(c, 2)["idx"])
    assert not torch.equal(a["idx"], b["idx"])


# ---- RoIAlign -------------------------------------------------------------------------------------------------------------------
def _roi_raw(RO, c, fill=SENTINEL, accumulate=False, gf=None):
    feat, gp = (_t(a) for a in RC.roi_inputs(c.Cf, c.PH, c.PW))
    rois, n_roi = _t(RC.ROIS), _t(RC.N_ROI)
    cs = RO.c_spec(RO.RcnnSpec(PH=c.PH, PW=c.PW, spatial_scale=RC.SCALE, sampling_ratio=c.ratio), B=RC.B, Cf=c.Cf, Hf=RC.HF, Wf=RC.WF,
                   S=RC.ROIS.shape[1])
    pooled = torch.full(gp.shape, fill, dtype=torch.float32, device=DEV)
    if gf is None:
        gf = torch.full(feat.shape, fill, dtype=torch.float32, device=DEV)
    lib = RO._lib()
    assert lib.gsr_roi_align(ctypes.byref(cs), feat.data_ptr(), rois.data_ptr(), n_roi.data_ptr(), 2, pooled.data_ptr(), _stream()) == 0, \
        lib.gsr_last_error()
    assert lib.gsr_roi_align_backward(ctypes.byref(cs), rois.data_ptr(), n_roi.data_ptr(), 2, gp.data_ptr(), gf.data_ptr(),
                                      1 if accumulate else 0, _stream()) == 0, lib.gsr_last_error()
    return dict(pooled=pooled, grad_features=gf)


@pytest.mark.parametrize("c", RC.ROI_CASES, ids=lambda c: c.id)
def test_roi_align_and_its_backward_match_the_oracle(RO, c):
    ref = RC.roi_reference(c)
    assert RC.roi_margins_ok(ref)
    got = _roi_raw(RO, c)
    for k in ("pooled", "grad_features"):
        assert not (got[k] == SENTINEL).any() and torch.isfinite(got[k]).all(), f"{c.id}: {k} holds unwritten elements"
    _check("device", c.id, got, ref, ("pooled", "grad_features"))
    assert (got["pooled"][0, 7] == 0).all() and (got["pooled"][1, 7:] == 0).all()


def test_roi_align_backward_repeats_accumulates_and_runs_on_a_side_stream(RO):
    c = RC.RoiCase(70, 7, 7, 0)
    first = _roi_raw(RO, c)
    again = _roi_raw(RO, c, fill=3.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _roi_raw(RO, c)
    side.synchronize()
    for k in ("pooled", "grad_features"):
        assert _bits(first[k]) == _bits(again[k]) == _bits(other[k])
    base = torch.arange(first["grad_features"].numel(), dtype=torch.float32, device=DEV).reshape(first["grad_features"].shape) * 0.25
    acc = _roi_raw(RO, c, accumulate=True, gf=base.clone())
    assert torch.equal(acc["grad_features"], base + first["grad_features"])


def test_roi_align_autograd_function(RO):
    c = RC.RoiCase(3, 3, 5, 2)
    ref = RC.roi_reference(c)
    assert RC.roi_margins_ok(ref)
    feat, gp = (_t(a) for a in RC.roi_inputs(c.Cf, c.PH, c.PW))
    f = feat.clone().requires_grad_(True)
    from gsplat_attack.roi_detector import roi_align
    pooled = roi_align(f, _t(RC.ROIS), _t(RC.N_ROI), (c.PH, c.PW), RC.SCALE, c.ratio)
    (pooled * gp * 2.0).sum().backward()
    raw = _roi_raw(RO, c)
    assert torch.equal(pooled.detach(), raw["pooled"])
    _check("autograd", c.id, dict(pooled=pooled.detach(), grad_features=f.grad / 2.0), ref, ("pooled", "grad_features"))
    # no counts: every finite row is pooled
    full = roi_align(feat[1:], _t(RC.ROIS)[1:], None, (c.PH, c.PW), RC.SCALE, c.ratio)
    assert float(full[0, 7].abs().max()) > 0 and (full[0, 8] == 0).all()


# ---- the loss -------------------------------------------------------------------------------------------------------------------
def _loss_spec(RO, c):
    return RO.RcnnSpec(beta=c.beta, w_cls=c.w[0], w_box=c.w[1], class_agnostic=c.agnostic)


def _loss_raw(RO, c, with_grads=True):
    i = RC.loss_inputs(c)
    x, d, r, lb, gr, gb = (_t(i[k]) for k in ("scores", "deltas", "rois", "labels", "gt_row", "gt_boxes"))
    cs = RO.c_spec(_loss_spec(RO, c), B=RC.B, M=RC.LOSS_M, C=c.C, S=RC.LOSS_S)
    ws = torch.empty(((RO.workspace_bytes(cs) + 15) // 16 * 2,), dtype=torch.int64, device=DEV)
    loss = torch.full((3,), SENTINEL, dtype=torch.float32, device=DEV)
    gs = torch.full(x.shape, SENTINEL, dtype=torch.float32, device=DEV) if with_grads else None
    gd = torch.full(d.shape, SENTINEL, dtype=torch.float32, device=DEV) if with_grads else None
    lib = RO._lib()
    rc = lib.gsr_rcnn_loss(ctypes.byref(cs), x.data_ptr(), d.data_ptr(), r.data_ptr(), lb.data_ptr(), gr.data_ptr(), gb.data_ptr(),
                           ws.data_ptr(), ws.numel() * 8, loss.data_ptr(), gs.data_ptr() if with_grads else None,
                           gd.data_ptr() if with_grads else None, _stream())
    assert rc == 0, lib.gsr_last_error()
    return dict(loss=loss, grad_scores=gs, grad_deltas=gd)


@pytest.mark.parametrize("c", RC.LOSS_CASES, ids=lambda c: c.id)
def test_loss_and_gradients_match_the_oracle(RO, c):
    ref = RC.loss_reference(c)
    got = _loss_raw(RO, c)
    for k in RC.LOSS_COMPARED:
        assert not (got[k] == SENTINEL).any() and torch.isfinite(got[k]).all(), f"{c.id}: {k} holds unwritten elements"
    _check("device", c.id, got, ref, RC.LOSS_COMPARED)
    assert _bits(_loss_raw(RO, c, with_grads=False)["loss"]) == _bits(got["loss"]) == _bits(_loss_raw(RO, c)["loss"])
    zr = RC.loss_inputs(c)["zero_row"]
    if zr is not None:
        assert (got["grad_deltas"][zr[0], zr[1]] == 0).all()


def test_loss_autograd_function_with_an_upstream_gradient(RO):
    c = RC.LOSS_CASES[1]
    ref, i = RC.loss_reference(c), RC.loss_inputs(c)
    x, d = _t(i["scores"]).requires_grad_(True), _t(i["deltas"]).requires_grad_(True)
    total, items = RO.rcnn_loss(x, d, _t(i["rois"]), _t(i["labels"]), _t(i["gt_row"]), _t(i["gt_boxes"]), _loss_spec(RO, c))
    (total * 2.0).backward()
    got = dict(loss=torch.cat([items, total.detach()[None]]), grad_scores=x.grad / 2.0, grad_deltas=d.grad / 2.0)
    _check("autograd", c.id, got, ref, RC.LOSS_COMPARED)
    assert not items.requires_grad


# ---- the output stage ---------------------------------------------------------------------------------------------------------
def _output(c):
    from gsplat_attack.roi_detector import RoIHeadOutput
    return RoIHeadOutput(RC.FRAME, conf=c.conf, iou=RC.IOU_THR, max_det=c.max_det, class_agnostic=c.agnostic)


@pytest.mark.parametrize("c", RC.POST_CASES, ids=lambda c: c.id)
def test_output_stage_equals_the_oracle_and_the_host_build(RO, host, c):
    o, h = RC.post_reference(c), RC.host_post(host, c)
    assert RC.post_margins_ok(o)
    scores, deltas, prop, n_prop = (_t(a) for a in RC.post_inputs(c))
    dets, counts = _output(c).detect(scores, deltas, prop, n_prop=n_prop)
    dets2, counts2 = _output(c).detect(scores, deltas, prop, n_prop=n_prop)
    assert _bits(dets) == _bits(dets2) and _bits(counts) == _bits(counts2)
    dn, cn = dets.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(cn, o["counts"]) and np.array_equal(cn, h["counts"])
    tol = 1e-4 * max(RC.FRAME)          # float32 boxes of up to 200 px through an exp and a few products: well under 1e-4 relative
    for b in range(RC.B):
        n = int(cn[b, 0])
        assert dn[b, :n, 5].astype(int).tolist() == o["classes"][b] == h["dets"][b, :n, 5].astype(int).tolist()
        for want in (o["dets"], h["dets"]):                               # the kept order: row by row the oracle's and the host's
            assert np.abs(dn[b, :, :5] - want[b, :, :5]).max() <= tol
        assert (dn[b, n:] == 0).all()


def test_verdicts_equal_a_host_restatement(RO):
    c = RC.POST_CASES[0]
    scores, deltas, prop, n_prop = (_t(a) for a in RC.post_inputs(c))
    out = _output(c)
    dets, counts = out.detect(scores, deltas, prop, n_prop=n_prop)
    dn, cn = dets.cpu().numpy(), counts.cpu().numpy()
    gts = [[[38.0, 29.0, 97.0, 88.0], [float("nan")] * 4], [[120.0, 90.0, 181.0, 151.0], [12.0, 12.0, 31.0, 29.0]]]
    for gt in gts:
        for target, untarget, targeted in ((0, -1, True), (2, 0, True), (1, 2, False), (0, 1, True)):
            flags, best = out.verdicts(scores, deltas, prop, torch.tensor(gt), target, untarget if untarget >= 0 else None, targeted,
                                       n_prop=n_prop)
            want = [RC.verdict_ref(dn[b], cn[b], gt[b], target, untarget, targeted) for b in range(RC.B)]
            assert flags.cpu().tolist() == want, (gt, target, untarget, targeted)
    flags, best = out.verdicts(scores, deltas, prop, None, 1, None, True, n_prop=n_prop)
    assert flags.cpu().tolist() == [RC.verdict_ref(dn[b], cn[b], None, 1, -1, True) for b in range(RC.B)] and (best == -1).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------
E_NC, E_CF, E_STRIDE, E_P = 3, 6, 8, 4      # classes; feature channels; a 64 x 64 render -> an 8 x 8 map; 4 x 4 pooling
GT = torch.tensor([[10.3, 12.6, 52.2, 49.7], [14.4, 7.7, 56.3, 54.1]])   # per view, render frame
TARGET = 1
PARAMS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")


class Net(torch.nn.Module):
    """A strided-convolution backbone, a fixed proposer (a grid of boxes plus shifted copies of two anchors) and a linear
    box head; fixed-seed weights."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(29)
        self.conv = torch.nn.Conv2d(3, E_CF, E_STRIDE, stride=E_STRIDE)
        self.fc = torch.nn.Linear(E_CF * E_P * E_P, (E_NC + 1) + 4 * E_NC)
        with torch.no_grad():
            for p, s in ((self.conv.weight, 0.08), (self.conv.bias, 0.3), (self.fc.weight, 0.05), (self.fc.bias, 0.3)):
                p.copy_(torch.randn(p.shape, generator=g) * s)
        cells = [[x, y, x + 20.0, y + 18.0] for y in (2.0, 22.0, 42.0) for x in (1.0, 21.0, 41.0)]
        near = [[12.0 + d, 10.0 + d, 50.0 + d, 52.0 - d] for d in (0.0, 2.0, 4.0)]
        self.register_buffer("boxes", torch.tensor(cells + near))

    def backbone(self, x):
        return torch.tanh(self.conv(x))

    def proposer(self, features):
        return self.boxes[None].expand(features.shape[0], -1, -1).contiguous()

    def box_head(self, pooled):
        o = self.fc(pooled.flatten(1))
        return o[:, :E_NC + 1], o[:, E_NC + 1:]


def _scene():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), width=64, height=64, n_views=2)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _loss_fn():
    from gsplat_attack.roi_detector import ProposalSampler, RoIHeadLoss, make_roi_loss_fn
    net = Net().to(DEV)
    sampler = ProposalSampler(E_NC, per_image=8, positive_fraction=0.25, seed=5)
    return make_roi_loss_fn(net.backbone, net.proposer, net.box_head, None, sampler, RoIHeadLoss(E_NC, cls=1.0, box=1.0), GT, TARGET,
                            output_size=(E_P, E_P), spatial_scale=1.0 / E_STRIDE), net


def test_loss_fn_gradients_reach_the_gaussians_and_repeat():
    from gsplat_attack.renderer import PipelineParams, render_batch
    model, cams, bg = _scene()
    loss_fn, _ = _loss_fn()
    raw = [model.named_parameters()[n] for n in PARAMS]
    runs = []
    for _ in range(2):
        model.zero_grad()
        renders = render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"]
        total = loss_fn(renders, idx=[0, 1])
        total.backward()
        runs.append([total.detach().clone()] + [p.grad.detach().clone() for p in raw])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0
        assert torch.equal(a, b)


def test_pgd_attack_with_the_roi_loss_repeats():
    from gsplat_attack.attack import pgd_attack
    hists, params = [], []
    for _ in range(2):
        model, cams, bg = _scene()
        loss_fn, _ = _loss_fn()
        hists.append(pgd_attack(model, cams, iters=3, groups=("color",), bg=bg, batch_loss=True, loss_fn=loss_fn))
        params.append([model.named_parameters()[n].detach().clone() for n in PARAMS])
    torch.cuda.synchronize()
    for h in hists:
        assert len(h) == 3 and all(np.isfinite(v) for v in h) and h[0] != h[1]     # the step moved the loss
    assert hists[0] == hists[1]
    assert all(torch.equal(a, b) for a, b in zip(params[0], params[1]))
    fresh = _scene()[0].named_parameters()
    assert not all(torch.equal(a, fresh[n].detach()) for a, n in zip(params[0], PARAMS))       # the attack moved the parameters

"""The FPN RoI pooler on the device: the cases of tests/fpn_cases.py.  The assignment integer-equal to the float64 oracle and to
the host build on sentinel-filled buffers; pooled values and every level's gradient within 4 x the float32 oracle's own error
(floor 2^-22, never above 1e-3) of the float64 oracle, the margins asserted first; pooled and every gradient bit for bit what
the single-level entries give on NaN-masked RoIs (no tolerance), with `accumulate` and with one level; the same bits on every
call and on a side stream; the autograd function; the size limits; and the pooler behind a four-map backbone, an RpnProposer
over four levels and a box head as pgd_attack's loss_fn, bit for bit repeatable."""
import ctypes

import numpy as np
import pytest
import torch

import fpn_cases as FC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
ISENT = -777


@pytest.fixture(scope="module")
def FO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import fpn_ops
    D._load()
    assert fpn_ops.available()
    return fpn_ops


@pytest.fixture(scope="module")
def host():
    return FC.host_lib()


def _t(a):
    return None if a is None else torch.tensor(np.array(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _spec(FO, c, nl=FC.NL):
    return FO.FpnSpec(scales=tuple(1.0 / s for s in FC.STRIDES[:nl]), thr=FC.THR[:nl], PH=c.PH, PW=c.PW, sampling_ratio=c.ratio,
                      canonical_size=FC.CANON_SIZE)


def _raw(FO, c, n_roi=FC.N_ROI, fill=SENTINEL, accumulate=False, grads=None, nl=FC.NL, rois=FC.ROIS, feats=None, gp=None, spec=None):
    """Both C entries on sentinel-filled caller buffers -> dict(pooled, roi_level, level_list, level_count, grad0..)."""
    if feats is None:
        feats, gp = FC.inputs(c.Cf, c.PH, c.PW)
    feats = [_t(f) for f in feats[:nl]]
    gp, r, n = _t(gp), _t(rois), _t(n_roi)
    Bn, S = int(r.shape[0]), int(r.shape[1])
    cs = FO.c_spec(_spec(FO, c, nl) if spec is None else spec, B=Bn, S=S, Cf=c.Cf, sizes=[tuple(f.shape[2:]) for f in feats])
    out = dict(pooled=torch.full((Bn, S, c.Cf, c.PH, c.PW), fill, dtype=torch.float32, device=DEV),
               roi_level=torch.full((Bn, S), ISENT, dtype=torch.int32, device=DEV),
               level_list=torch.full((Bn, nl, S), ISENT, dtype=torch.int32, device=DEV),
               level_count=torch.full((Bn, nl), ISENT, dtype=torch.int32, device=DEV))
    if grads is None:
        grads = [torch.full(f.shape, fill, dtype=torch.float32, device=DEV) for f in feats]
    lib = FO._lib()
    fp = (ctypes.c_void_p * nl)(*[f.data_ptr() for f in feats])
    gpp = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in grads])
    rc = lib.gsr_fpn_pool(ctypes.byref(cs), fp, r.data_ptr(), None if n is None else n.data_ptr(), 2, out["pooled"].data_ptr(),
                          out["roi_level"].data_ptr(), out["level_list"].data_ptr(), out["level_count"].data_ptr(), _stream())
    assert rc == 0, lib.gsr_last_error()
    rc = lib.gsr_fpn_pool_backward(ctypes.byref(cs), r.data_ptr(), out["level_list"].data_ptr(), out["level_count"].data_ptr(),
                                   gp.data_ptr(), gpp, 1 if accumulate else 0, _stream())
    assert rc == 0, lib.gsr_last_error()
    out.update({f"grad{l}": g for l, g in enumerate(grads)})
    return out


# ---- 1. the assignment ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_roi", (FC.N_ROI, FC.N_ROI_ZERO, None), ids=("counts", "count-0", "no-counts"))
def test_assignment_equals_the_oracle_and_the_host_build(FO, host, n_roi):
    assert FC.check_declarations()
    lv, lists, counts = FC.oracle_levels(FC.ROIS, n_roi, 2)
    h = FC.host_assign(host, n_roi=n_roi)
    got = _raw(FO, FC.CASES[0], n_roi=n_roi)
    g_lv, g_ll, g_lc = (got[k].cpu().numpy() for k in ("roi_level", "level_list", "level_count"))
    assert not (g_lv == ISENT).any() and not (g_lc == ISENT).any()
    assert np.array_equal(g_lv, lv) and np.array_equal(g_lv, h["roi_level"])
    assert np.array_equal(g_lc, counts) and np.array_equal(g_lc, h["level_count"])
    assert FC.lists_equal(g_ll, g_lc, lists)
    listed = set()
    for b in range(FC.B):
        for l in range(FC.NL):
            n = int(counts[b, l])
            row = g_ll[b, l, :n].tolist()
            assert row == sorted(row) and row == h["level_list"][b, l, :n].tolist()
            listed |= {(b, s) for s in row}
    dead = {(b, s) for b in range(FC.B) for s in range(FC.S) if lv[b, s] == -1}
    assert dead and not dead & listed
    assert lv[0, len(FC.TABLE)] == lv[0, len(FC.TABLE) + 1] == -1                     # the NaN row and the inf row
    if n_roi is FC.N_ROI_ZERO:
        assert (g_lc[1] == 0).all() and (got["pooled"][1] == 0).all()
        for l in range(FC.NL):
            assert (got[f"grad{l}"][1] == 0).all()


# ---- 2. oracle parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FC.CASES, ids=lambda c: c.id)
def test_pooled_and_gradients_match_the_oracle(FO, c):
    ref = FC.reference(c)
    assert FC.margins_ok(ref)
    got = _raw(FO, c)
    fails = []
    for k in FC.COMPARED:
        assert not (got[k] == SENTINEL).any() and torch.isfinite(got[k]).all(), f"{c.id}: {k} holds unwritten elements"
        e, y = FC.err(got[k], ref["o64"][k]), ref["yard"][k]
        b = FC.bound(y)
        print(f"device {c.id} {k}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {b:.3e}")
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, f"{c.id}: {fails}"
    lv, _, counts = FC.oracle_levels(FC.ROIS, FC.N_ROI, 2)
    assert (got["pooled"][_t(lv == -1)] == 0).all()
    assert counts[1, FC.NL - 1] == 0 and (got[f"grad{FC.NL - 1}"][1] == 0).all()       # a level that received no RoI
    b, s = FC.INVERTED                                                                  # backwards at a fixed ratio, grid 0 when adaptive
    assert lv[b, s] == 0 and (float(got["pooled"][b, s].abs().max()) > 0) == (c.ratio > 0)


def test_exact_edges_by_hand(FO, host):
    """The samples exactly at -1 and at n (valid: the border cell with weight 1) and the next positions further out (0) through
    the pooler's kernels, on a one-level pyramid of stride 1: the values rcnn_cases.roi_edge_inputs writes out by hand, and the
    host build's bits."""
    c, _, (feat, gp, rois, n_roi), pooled, gf = FC.edge_inputs()
    spec = FO.FpnSpec(scales=(1.0,), thr=(0.0,), PH=c.PH, PW=c.PW, sampling_ratio=c.ratio, canonical_size=FC.CANON_SIZE)
    got = _raw(FO, c, n_roi=n_roi, nl=1, rois=rois, feats=(feat,), gp=gp, spec=spec)
    h_p, h_g = FC.host_pool_edges(host)
    assert (got["roi_level"] == 0).all()
    assert np.array_equal(got["pooled"].cpu().numpy()[0, :, :, 0, 0], pooled) and _bits(got["pooled"]) == h_p.tobytes()
    assert np.array_equal(got["grad0"].cpu().numpy()[0], gf) and _bits(got["grad0"]) == h_g.tobytes()


# ---- 3. bit for bit the single-level entries ----------------------------------------------------------------------------------
def _single_level(c, n_roi, nl=FC.NL, base=None):
    """pooled as the sum over levels of roi_align_forward on NaN-masked RoIs, and roi_align_backward per level."""
    from diff_gaussian_rasterization import rcnn_ops as RO
    feats, gp = FC.inputs(c.Cf, c.PH, c.PW)
    thr = FC.THR[:nl]
    lv, _, _ = FC.oracle_levels(FC.ROIS, n_roi, 2, thr=thr)
    n, gpt = _t(n_roi), _t(gp)
    pooled, grads, nonzero = None, [], torch.zeros((FC.B, FC.S), dtype=torch.int32, device=DEV)
    for l in range(nl):
        spec = RO.RcnnSpec(PH=c.PH, PW=c.PW, spatial_scale=1.0 / FC.STRIDES[l], sampling_ratio=c.ratio)
        r = _t(FC.masked_rois(FC.ROIS, lv, l))
        p = RO.roi_align_forward(_t(feats[l]), r, n, spec)
        nonzero += (p.flatten(2) != 0).any(-1).int()
        pooled = p if pooled is None else pooled + p
        out = None if base is None else base[l].clone()
        grads.append(RO.roi_align_backward(gpt, r, n, feats[l].shape, spec, out=out, accumulate=base is not None))
    assert int(nonzero.max()) == 1                                                    # exactly one addend per row is non-zero
    return pooled, grads


@pytest.mark.parametrize("c", FC.CASES, ids=lambda c: c.id)
def test_bitwise_equal_to_the_single_level_entries(FO, c):
    got = _raw(FO, c)
    pooled, grads = _single_level(c, FC.N_ROI)
    assert _bits(got["pooled"]) == _bits(pooled)
    for l in range(FC.NL):
        assert _bits(got[f"grad{l}"]) == _bits(grads[l]), f"level {l}"
    # accumulate onto a non-zero out
    base = [torch.arange(g.numel(), dtype=torch.float32, device=DEV).reshape(g.shape) * 0.25 - 3.0 for g in grads]
    acc = _raw(FO, c, accumulate=True, grads=[b.clone() for b in base])
    _, want = _single_level(c, FC.N_ROI, base=base)
    for l in range(FC.NL):
        assert _bits(acc[f"grad{l}"]) == _bits(want[l]), f"accumulate, level {l}"
        assert torch.equal(acc[f"grad{l}"], base[l] + grads[l])


@pytest.mark.parametrize("c", FC.CASES, ids=lambda c: c.id)
def test_one_level_equals_roi_align(FO, c):
    """nl = 1: every live finite row is of level 0, so the entry is gsr_roi_align and gsr_roi_align_backward on the RoIs as they are."""
    from diff_gaussian_rasterization import rcnn_ops as RO
    feats, gp = FC.inputs(c.Cf, c.PH, c.PW)
    got = _raw(FO, c, nl=1)
    spec = RO.RcnnSpec(PH=c.PH, PW=c.PW, spatial_scale=1.0 / FC.STRIDES[0], sampling_ratio=c.ratio)
    r, n = _t(FC.ROIS), _t(FC.N_ROI)
    assert _bits(got["pooled"]) == _bits(RO.roi_align_forward(_t(feats[0]), r, n, spec))
    assert _bits(got["grad0"]) == _bits(RO.roi_align_backward(_t(gp), r, n, feats[0].shape, spec))
    lv = got["roi_level"].cpu().numpy()
    assert set(np.unique(lv)) == {-1, 0} and np.array_equal(lv, FC.oracle_levels(FC.ROIS, FC.N_ROI, 2, thr=(0.0,))[0])


# ---- 4. repeatability and autograd ----------------------------------------------------------------------------------------------
def test_same_bits_again_and_on_a_side_stream(FO):
    c = FC.Case(70, 7, 7, 0)
    first = _raw(FO, c)
    again = _raw(FO, c, fill=3.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _raw(FO, c)
    side.synchronize()
    for k in FC.COMPARED + ("roi_level", "level_count"):
        assert _bits(first[k]) == _bits(again[k]) == _bits(other[k]), k


def test_autograd_function_and_dtype_round_trip(FO):
    c = FC.Case(3, 3, 5, 2)
    feats, gp = FC.inputs(c.Cf, c.PH, c.PW)
    spec = _spec(FO, c)
    fs = [_t(f).requires_grad_(True) for f in feats]
    r, n, gpt = _t(FC.ROIS), _t(FC.N_ROI), _t(gp)
    pooled = FO.fpn_pool(fs, r, n, spec)
    (pooled * gpt * 2.0).sum().backward()
    raw = _raw(FO, c)
    assert torch.equal(pooled.detach(), raw["pooled"])
    p2, lv, ll, lc = FO.pool_forward([f.detach() for f in fs], r, n, spec)
    want = FO.pool_backward(gpt * 2.0, r, ll, lc, [f.shape for f in fs], spec)
    for l in range(FC.NL):
        assert torch.equal(fs[l].grad, want[l]), l
    assert torch.equal(p2, raw["pooled"]) and torch.equal(lv, raw["roi_level"])
    assert not r.requires_grad
    # float16 features: converted on the way in, the gradients cast back
    hs = [_t(f).half().requires_grad_(True) for f in feats]
    ph = FO.fpn_pool(hs, r, n, spec)
    assert ph.dtype == torch.float32
    (ph * gpt).sum().backward()
    p32, _, ll, lc = FO.pool_forward([h.detach().float() for h in hs], r, n, spec)
    w32 = FO.pool_backward(gpt, r, ll, lc, [f.shape for f in fs], spec)
    assert torch.equal(ph.detach(), p32)
    for l in range(FC.NL):
        assert hs[l].grad.dtype == torch.float16 and torch.equal(hs[l].grad, w32[l].half())
    # the public pooler: the same pooled bits and the levels
    from gsplat_attack.roi_detector import FpnRoIPooler
    pooler = FpnRoIPooler(FC.STRIDES, output_size=(c.PH, c.PW), sampling_ratio=c.ratio)
    assert torch.equal(pooler([f.detach() for f in fs], r, n), raw["pooled"])
    assert torch.equal(pooler.levels(r, n), raw["roi_level"])


# ---- 5. size limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1024, 1))
def test_size_limits(FO, host, S):
    rs = np.random.RandomState(5 + S)
    # sides whose sqrt(area) / 224 keeps 3 % away from every threshold: log2 of the size uniform, rejected near a power of two
    e = rs.uniform(4.2, 9.8, size=(FC.B, S))
    e = np.where(np.abs(e - np.round(e)) < 0.05, e + 0.1, e)
    size = 2.0 ** e * (224.0 / 256.0)
    asp = 2.0 ** rs.uniform(-1.0, 1.0, size=(FC.B, S))
    w, h = size * np.sqrt(asp), size / np.sqrt(asp)
    x0, y0 = rs.uniform(-20, 400, size=(FC.B, S)), rs.uniform(-20, 300, size=(FC.B, S))
    rois = np.stack([x0, y0, x0 + w, y0 + h], -1).astype(np.float32)
    if S > 1:
        rois[0, 5], rois[1, 700] = FC.NAN, FC.INF
    n_roi = np.array([[S, 0], [S - S // 4, 0]], np.int32)
    lv, lists, counts = FC.oracle_levels(rois, n_roi, 2)
    q = FC.level_q(rois)
    live = lv >= 0
    assert min(abs(q[live] - t).min() / t for t in FC.THR[1:]) > FC.GAP
    c = FC.Case(3, 2, 2, 1)
    feats = tuple(rs.standard_normal((FC.B, c.Cf, hh, ww)).astype(np.float32) for hh, ww in FC.SIZES)
    gp = rs.standard_normal((FC.B, S, c.Cf, c.PH, c.PW)).astype(np.float32)
    got = _raw(FO, c, n_roi=n_roi, rois=rois, feats=feats, gp=gp)
    h_ = FC.host_assign(host, rois=rois, n_roi=n_roi)
    g_lv, g_ll, g_lc = (got[k].cpu().numpy() for k in ("roi_level", "level_list", "level_count"))
    assert np.array_equal(g_lv, lv) and np.array_equal(g_lv, h_["roi_level"]) and np.array_equal(g_lc, counts)
    assert FC.lists_equal(g_ll, g_lc, lists)
    if S > 1:
        assert (counts > 64).all()                                                    # every list spans several waves
    for k in FC.COMPARED:
        assert not (got[k] == SENTINEL).any() and torch.isfinite(got[k]).all(), k
    assert (got["pooled"][_t(lv == -1)] == 0).all()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
E_NC, E_CF, E_P, E_A = 3, 6, 4, 3
E_STRIDES = (2, 4, 8, 16)                                                             # a 64 x 64 render -> maps of 32, 16, 8 and 4 cells
GT = torch.tensor([[10.3, 12.6, 52.2, 49.7], [14.4, 7.7, 56.3, 54.1]])   # per view, render frame
TARGET = 1
PARAMS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")


class Net(torch.nn.Module):
    """Four strided convolutions as a backbone, a 1 x 1 RPN head shared by the levels and a linear box head; fixed-seed weights."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(37)
        self.convs = torch.nn.ModuleList([torch.nn.Conv2d(3, E_CF, s, stride=s) for s in E_STRIDES])
        self.rpn = torch.nn.Conv2d(E_CF, 5 * E_A, 1)
        self.fc = torch.nn.Linear(E_CF * E_P * E_P, (E_NC + 1) + 4 * E_NC)
        with torch.no_grad():
            for conv in self.convs:
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (0.6 / conv.kernel_size[0]))
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.3)
            for p, s in ((self.rpn.weight, 0.8), (self.rpn.bias, 0.2), (self.fc.weight, 0.05), (self.fc.bias, 0.3)):
                p.copy_(torch.randn(p.shape, generator=g) * s)

    def backbone(self, x):
        return [torch.tanh(conv(x)) for conv in self.convs]

    def rpn_head(self, features):
        outs = [self.rpn(f) for f in features]
        return [o[:, :E_A] for o in outs], [0.3 * o[:, E_A:] for o in outs]

    def box_head(self, pooled):
        o = self.fc(pooled.flatten(1))
        return o[:, :E_NC + 1], o[:, E_NC + 1:]


def _scene():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), width=64, height=64, n_views=2)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _loss_fn():
    from gsplat_attack.proposals import RpnProposer, cell_anchors
    from gsplat_attack.roi_detector import FpnRoIPooler, ProposalSampler, RoIHeadLoss, make_roi_loss_fn
    net = Net().to(DEV)
    proposer = RpnProposer([(cell_anchors((size,), (0.5, 1.0, 2.0)), s, 0.0) for size, s in zip((8, 16, 32, 48), E_STRIDES)], (64.0, 64.0),
                           pre_topk=100, post_topk=100, nms=0.3, head=net.rpn_head)
    pooler = FpnRoIPooler(E_STRIDES, output_size=E_P, canonical_size=32.0, canonical_level=3)     # 16 px -> level 1, 32 -> 2, 64 -> 3
    sampler = ProposalSampler(E_NC, per_image=16, positive_fraction=0.25, seed=5)
    loss_fn = make_roi_loss_fn(net.backbone, proposer, net.box_head, None, sampler, RoIHeadLoss(E_NC, cls=1.0, box=1.0), GT, TARGET,
                               pooler=pooler)
    return loss_fn, net, proposer, pooler, sampler


def test_loss_fn_gradients_reach_the_gaussians_and_repeat():
    from gsplat_attack.renderer import PipelineParams, render_batch
    model, cams, bg = _scene()
    loss_fn, net, proposer, pooler, sampler = _loss_fn()
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
    # the RoIs the loss pooled came from more than one level
    with torch.no_grad():
        feats = net.backbone(renders)
        boxes, counts = proposer(feats)
        smp = sampler.sample(boxes, GT, torch.full((2,), TARGET), n_prop=counts)
        lv = pooler.levels(smp.rois, smp.counts).cpu().numpy()
    assert len(set(lv[lv >= 0].tolist())) >= 2


def test_pgd_attack_with_the_fpn_pooler_repeats():
    from gsplat_attack.attack import pgd_attack
    hists, params = [], []
    for _ in range(2):
        model, cams, bg = _scene()
        loss_fn = _loss_fn()[0]
        hists.append(pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=True, loss_fn=loss_fn))
        params.append([model.named_parameters()[n].detach().clone() for n in PARAMS])
    torch.cuda.synchronize()
    for h in hists:
        assert len(h) == 2 and all(np.isfinite(v) for v in h) and h[0] != h[1]     # the step moved the loss
    assert hists[0] == hists[1]
    assert all(torch.equal(a, b) for a, b in zip(params[0], params[1]))

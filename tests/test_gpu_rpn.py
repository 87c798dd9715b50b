"""The RPN proposal stage on the device: every case of tests/rpn_cases.py through the C entries on sentinel-filled buffers
(every output element written; kept slots, counts, levels and scores equal to the oracle and to the host build; boxes within
the float32 yardstick's bound; the oracle's margins asserted first), the same bits on a second call and on a side stream, two
levels chained through cand_offset against separate calls put together, RpnProposer against the raw entries, and the stage
behind a small torch backbone and RPN head as pgd_attack's loss_fn, bit for bit repeatable."""
import ctypes

import numpy as np
import pytest
import torch

import rpn_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
ISENT = -777


@pytest.fixture(scope="module")
def PO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import rpn_ops
    D._load()
    assert rpn_ops.available()
    return rpn_ops


def _t(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_nms(PO, cb, csc, cl, thr, post):
    """gsr_rpn_nms on sentinel-filled caller buffers; cb, csc, cl: device tensors."""
    B, N = csc.shape
    cs = PO.c_spec(PO.RpnSpec(post_topk=post, iou_thr=thr), B=B, N=N)
    n = ctypes.c_int64(0)
    lib = PO._lib()
    assert lib.gsr_rpn_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0
    ws = torch.full(((n.value + 7) // 8,), -1, dtype=torch.int64, device=DEV)
    out = dict(proposals=torch.full((B, post, 4), SENTINEL, dtype=torch.float32, device=DEV),
               scores=torch.full((B, post), SENTINEL, dtype=torch.float32, device=DEV),
               keep=torch.full((B, post), ISENT, dtype=torch.int32, device=DEV),
               counts=torch.full((B,), ISENT, dtype=torch.int32, device=DEV))
    rc = lib.gsr_rpn_nms(ctypes.byref(cs), cb.data_ptr(), csc.data_ptr(), cl.data_ptr(), ws.data_ptr(), n.value, out["proposals"].data_ptr(),
                         out["scores"].data_ptr(), out["keep"].data_ptr(), out["counts"].data_ptr(), _stream())
    assert rc == 0, lib.gsr_last_error()
    return out


def _raw_select(PO, c, levels=None, N=None, offsets=None):
    """gsr_rpn_select for the given levels of case c (default: all, chained) into sentinel-filled candidate arrays."""
    lvs, sizes = PC.inputs(c), PC.slots_of(c)
    levels = list(range(len(lvs))) if levels is None else levels
    N = sum(sizes) if N is None else N
    offsets = [sum(sizes[:l]) for l in levels] if offsets is None else offsets
    cb = torch.full((c.B, N, 4), SENTINEL, dtype=torch.float32, device=DEV)
    csc = torch.full((c.B, N), SENTINEL, dtype=torch.float32, device=DEV)
    cl = torch.full((c.B, N), ISENT, dtype=torch.int32, device=DEV)
    lib = PO._lib()
    for l, off in zip(levels, offsets):
        lv, ls = lvs[l], c.levels[l]
        cs = PO.c_spec(PO.RpnSpec(img_w=c.frame[0], img_h=c.frame[1], min_size=c.min_size, pre_topk=c.pre_topk, post_topk=1), B=c.B,
                       A=ls.A, Hf=ls.Hf, Wf=ls.Wf, stride=ls.stride, shift0=lv.shift0, level=l, cand_offset=off, N=N)
        lg, dl, ca = _t(lv.logits), _t(lv.deltas), _t(lv.cell)
        rc = lib.gsr_rpn_select(ctypes.byref(cs), lg.data_ptr(), dl.data_ptr(), ca.data_ptr(), cb.data_ptr(), csc.data_ptr(), cl.data_ptr(),
                                _stream())
        assert rc == 0, lib.gsr_last_error()
    return cb, csc, cl


def _written(out, who):
    for k, v in out.items():
        g = v.cpu().numpy()
        assert not (g == (ISENT if g.dtype == np.int32 else np.float32(SENTINEL))).any(), f"{who}: {k} holds unwritten elements"


@pytest.mark.parametrize("c", PC.NMS_CASES, ids=lambda c: c.id)
def test_nms_equals_the_oracle_and_the_host_build(PO, c):
    bx, sc, lv, thr, post = PC.nms_inputs(c)
    ref, host = PC.nms_reference(c), PC.host_nms(PC.host_lib(), bx, sc, lv, thr, post)
    got = _raw_nms(PO, _t(bx), _t(sc), _t(lv), thr, post)
    _written(got, c.id)
    for k in ("counts", "keep"):
        g = got[k].cpu().numpy()
        assert np.array_equal(g, ref[k]) and np.array_equal(g, host[k]), f"{c.id}: {k} differs"
    assert _bits(got["scores"]) == ref["scores"].tobytes() == host["scores"].tobytes()
    assert _bits(got["proposals"]) == ref["proposals"].astype(np.float32).tobytes() == host["proposals"].tobytes()


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_select_and_nms_equal_the_oracle_and_the_host_build(PO, c):
    ref, host = PC.reference(c), PC.host_propose(c)
    assert PC.margins_ok(c, ref)
    cb, csc, cl = _raw_select(PO, c)
    _written(dict(cand_boxes=cb, cand_scores=csc, cand_level=cl), c.id)
    g_level = cl.cpu().numpy()
    assert np.array_equal(g_level, ref["cand_level"]) and np.array_equal(g_level, host["cand_level"]), f"{c.id}: levels differ"
    assert _bits(csc) == ref["cand_scores"].tobytes() == host["cand_scores"].tobytes(), f"{c.id}: scores (hence ranks) differ"
    PC.box_check(f"gpu {c.id} cand_boxes", cb.cpu().numpy(), ref["cand_boxes"], ref["cand_boxes32"])
    if c.exact:
        assert _bits(cb) == ref["cand_boxes"].astype(np.float32).tobytes()
    got = _raw_nms(PO, cb, csc, cl, c.thr, c.post)
    _written(got, c.id)
    n = ref["nms"]
    for k in ("counts", "keep"):
        g = got[k].cpu().numpy()
        assert np.array_equal(g, n[k]) and np.array_equal(g, host["nms"][k]), f"{c.id}: {k} differs"
    assert _bits(got["scores"]) == n["scores"].tobytes()
    PC.box_check(f"gpu {c.id} proposals", got["proposals"].cpu().numpy(), n["proposals"], PC.proposals32(ref))


BY = {c.id: c for c in PC.CASES}


@pytest.mark.parametrize("cid", ["c4-thr75-post2000", "float-two-levels"])
def test_same_bits_again_and_on_a_side_stream(PO, cid):
    c = BY[cid]

    def run():
        cand = _raw_select(PO, c)
        out = _raw_nms(PO, *cand, c.thr, c.post)
        return [_bits(t) for t in cand] + [_bits(out[k]) for k in ("proposals", "scores", "keep", "counts")]

    first, second = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert first == second == third


def test_two_levels_chained_equal_the_levels_put_together(PO):
    c = BY["two-levels"]
    n0, n1 = PC.slots_of(c)
    chained = _raw_select(PO, c)
    a = _raw_select(PO, c, levels=[0], N=n0, offsets=[0])
    b = _raw_select(PO, c, levels=[1], N=n1, offsets=[0])
    together = [torch.cat([x, y], 1).contiguous() for x, y in zip(a, b)]
    assert [_bits(t) for t in chained] == [_bits(t) for t in together]
    one, two = _raw_nms(PO, *chained, c.thr, c.post), _raw_nms(PO, *together, c.thr, c.post)
    assert all(_bits(one[k]) == _bits(two[k]) for k in one)
    # a level writes its own range and nothing else
    only1 = _raw_select(PO, c, levels=[1])
    assert (only1[2][:, :n0] == ISENT).all() and (only1[0][:, :n0] == SENTINEL).all() and _bits(only1[2][:, n0:]) == _bits(chained[2][:, n0:])


@pytest.mark.parametrize("cid", ["two-levels", "float-min16", "short-level"])
def test_proposer_equals_the_raw_entries(PO, cid):
    from gsplat_attack.proposals import RpnProposer
    c = BY[cid]
    lvs = PC.inputs(c)
    raw = _raw_nms(PO, *_raw_select(PO, c), c.thr, c.post)
    prop = RpnProposer([(torch.tensor(lv.cell), lv.stride, 0.0) for lv in lvs], c.frame, pre_topk=c.pre_topk, post_topk=c.post, nms=c.thr,
                       min_size=c.min_size)
    lg, dl = [_t(lv.logits) for lv in lvs], [_t(lv.deltas) for lv in lvs]
    p = prop.propose(lg, dl) if len(lvs) > 1 else prop.propose(lg[0], dl[0])
    assert _bits(p.boxes) == _bits(raw["proposals"]) and _bits(p.scores) == _bits(raw["scores"]) and _bits(p.counts) == _bits(raw["counts"])
    out, cand = PO.propose([PO.Level(l, d, _t(lv.cell), lv.stride) for l, d, lv in zip(lg, dl, lvs)],
                           PO.RpnSpec(c.frame[0], c.frame[1], c.min_size, c.pre_topk, c.post, c.thr), return_candidates=True)
    assert _bits(out.keep) == _bits(raw["keep"]) and _bits(cand[2]) == PC.reference(c)["cand_level"].tobytes()


# ---- end to end -------------------------------------------------------------------------------------------------------------
E_NC, E_CF, E_STRIDE, E_P, E_A = 3, 6, 8, 4, 3     # classes; feature channels; a 64 x 64 render -> an 8 x 8 map; 4 x 4 pooling
GT = torch.tensor([[10.3, 12.6, 52.2, 49.7], [14.4, 7.7, 56.3, 54.1]])   # per view, render frame
TARGET = 1
PARAMS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")


class Net(torch.nn.Module):
    """A strided-convolution backbone, a 1 x 1 RPN head (A objectness logits and 4A deltas per cell) and a linear box head;
    fixed-seed weights."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(31)
        self.conv = torch.nn.Conv2d(3, E_CF, E_STRIDE, stride=E_STRIDE)
        self.rpn = torch.nn.Conv2d(E_CF, 5 * E_A, 1)
        self.fc = torch.nn.Linear(E_CF * E_P * E_P, (E_NC + 1) + 4 * E_NC)
        with torch.no_grad():
            for p, s in ((self.conv.weight, 0.08), (self.conv.bias, 0.3), (self.rpn.weight, 0.8), (self.rpn.bias, 0.2),
                         (self.fc.weight, 0.05), (self.fc.bias, 0.3)):
                p.copy_(torch.randn(p.shape, generator=g) * s)

    def backbone(self, x):
        return torch.tanh(self.conv(x))

    def rpn_head(self, features):
        o = self.rpn(features)
        return o[:, :E_A], 0.3 * o[:, E_A:]

    def box_head(self, pooled):
        o = self.fc(pooled.flatten(1))
        return o[:, :E_NC + 1], o[:, E_NC + 1:]


def _scene():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), width=64, height=64, n_views=2)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _proposer(net):
    from gsplat_attack.proposals import RpnProposer, cell_anchors
    return RpnProposer([(cell_anchors((24,), (0.5, 1.0, 2.0)), E_STRIDE, 0.0)], (64.0, 64.0), pre_topk=100, post_topk=100, nms=0.3,
                       head=net.rpn_head)


def _loss_fn(proposer_of=_proposer):
    from gsplat_attack.roi_detector import ProposalSampler, RoIHeadLoss, make_roi_loss_fn
    net = Net().to(DEV)
    sampler = ProposalSampler(E_NC, per_image=8, positive_fraction=0.25, seed=5)
    return make_roi_loss_fn(net.backbone, proposer_of(net), net.box_head, None, sampler, RoIHeadLoss(E_NC, cls=1.0, box=1.0), GT, TARGET,
                            output_size=(E_P, E_P), spatial_scale=1.0 / E_STRIDE), net


def test_pgd_attack_with_an_rpn_proposer_repeats():
    from gsplat_attack.attack import pgd_attack
    hists, params = [], []
    for _ in range(2):
        model, cams, bg = _scene()
        loss_fn, _ = _loss_fn()
        hists.append(pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=True, loss_fn=loss_fn))
        params.append([model.named_parameters()[n].detach().clone() for n in PARAMS])
    torch.cuda.synchronize()
    for h in hists:
        assert len(h) == 2 and all(np.isfinite(v) for v in h) and h[0] != h[1]     # the step moved the loss
    assert hists[0] == hists[1]
    assert all(torch.equal(a, b) for a, b in zip(params[0], params[1]))


def test_the_count_reaches_the_sampler_and_a_plain_tensor_is_as_before():
    from gsplat_attack.renderer import PipelineParams, render_batch
    from gsplat_attack.roi_detector import ProposalSampler, RoIHeadLoss, roi_align
    model, cams, bg = _scene()
    with torch.no_grad():
        renders = render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"]
    counted, net = _loss_fn()
    prop = _proposer(net)
    boxes, counts = prop(net.backbone(renders))
    assert int(counts.min()) >= 1 and int(counts.max()) < boxes.shape[1]            # zero rows beyond the count exist
    plain, _ = _loss_fn(lambda n: (lambda f: _proposer(n)(f)[0]))                  # the same boxes as one tensor
    full, _ = _loss_fn(lambda n: (lambda f: (_proposer(n)(f)[0], None)))
    with torch.no_grad():
        l_counted, l_plain, l_full = counted(renders, idx=[0, 1]), plain(renders, idx=[0, 1]), full(renders, idx=[0, 1])
        # the chain as it was before proposers could return a count: every row of the tensor is a proposal
        features = net.backbone(renders)
        sampler, head_loss = ProposalSampler(E_NC, per_image=8, positive_fraction=0.25, seed=5), RoIHeadLoss(E_NC, cls=1.0, box=1.0)
        smp = sampler.sample(boxes, GT, torch.full((2,), TARGET, dtype=torch.int32))
        pooled = roi_align(features, smp.rois, smp.counts, (E_P, E_P), 1.0 / E_STRIDE, 0)
        scores, deltas = net.box_head(pooled.reshape(2 * 8, *pooled.shape[2:]))
        before = head_loss.loss(scores.reshape(2, 8, -1), deltas.reshape(2, 8, -1), smp, GT)[0]
        # with the count, no row beyond it is drawn
        smp_c = sampler.sample(boxes, GT, torch.full((2,), TARGET, dtype=torch.int32), n_prop=counts)
    assert torch.equal(l_plain, before) and torch.equal(l_full, before)
    for b in range(2):
        idx = smp_c.idx[b][: int(smp_c.counts[b, 0])]
        assert bool(((idx < int(counts[b])) | (idx >= boxes.shape[1])).all())      # a proposal below the count, or an appended gt row
    assert torch.isfinite(l_counted) and float(l_counted) > 0

"""The RPN loss stage on the device: every case of tests/rpnloss_cases.py through the C entries on sentinel-filled buffers
(every output element written; pre-labels, labels, matched rows and counts equal to the oracle and to the host build; loss and
both gradients within 4 x the float32 oracle's error, floor 2^-22, cap 1e-3; the oracle's margins asserted first), the same
bits on a second call and on a side stream, levels passed together against the same anchors as one level, RpnLoss against
the raw entries, the autograd wrapper under a non-unit upstream gradient, and the stage inside make_roi_loss_fn as
pgd_attack's loss_fn: bit for bit repeatable, with a gradient at the RPN head's weights.

Measured err / yardstick ratios of the kernels (MI355X) are recorded in DESIGN.md, section "RPN loss stage"."""
import ctypes

import numpy as np
import pytest
import torch

import rpnloss_cases as RC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def RO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import rpnloss_ops
    D._load()
    assert rpnloss_ops.available()
    return rpnloss_ops


@pytest.fixture(scope="module")
def host():
    return RC.host_lib()


def _t(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pp(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ws(RO, cs):
    n = ctypes.c_int64(0)
    assert RO._lib().gsr_rpnloss_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0
    return torch.full(((n.value + 15) // 16 * 2,), -1, dtype=torch.int64, device=DEV), n.value


def _raw_label(RO, c, ref):
    """gsr_rpnloss_label on sentinel-filled caller buffers."""
    inp = ref["inp"]
    cs = RC.c_spec(c, M=inp["gt"].shape[1])
    cells = [_t(a) for a in RC.cell_arrays(c)]
    ws, n = _ws(RO, cs)
    R = RC.total(c)
    out = {k: torch.full((c.B, R), RC.ISENT, dtype=torch.int32, device=DEV) for k in ("pre", "labels", "matched")}
    out["counts"] = torch.full((c.B, 4), RC.ISENT, dtype=torch.int32, device=DEV)
    gt, cls = _t(inp["gt"]), _t(inp["cls"])
    lib = RO._lib()
    rc = lib.gsr_rpnloss_label(ctypes.byref(cs), _pp(cells), gt.data_ptr(), cls.data_ptr(), ws.data_ptr(), n, out["labels"].data_ptr(),
                               out["matched"].data_ptr(), out["counts"].data_ptr(), out["pre"].data_ptr(), _stream())
    assert rc == 0, lib.gsr_last_error()
    return out


def _raw_loss(RO, c, ref, labels=None, matched=None, grads=True):
    """gsr_rpnloss on sentinel-filled caller buffers -> dict(loss, grad_logits, grad_deltas flat over the levels)."""
    inp, lab = ref["inp"], ref["lab"]
    cs = RC.c_spec(c, M=inp["gt"].shape[1])
    cells = [_t(a) for a in RC.cell_arrays(c)]
    ws, n = _ws(RO, cs)
    lg, dl = [_t(x) for x in inp["logits"]], [_t(d) for d in inp["deltas"]]
    gl, gd = [torch.full_like(x, RC.FSENT) for x in lg], [torch.full_like(d, RC.FSENT) for d in dl]
    loss = torch.full((3,), RC.FSENT, dtype=torch.float32, device=DEV)
    lb = _t(lab["labels"]) if labels is None else labels
    mt = _t(lab["matched"]) if matched is None else matched
    gt = _t(inp["gt"])
    lib = RO._lib()
    rc = lib.gsr_rpnloss(ctypes.byref(cs), lb.data_ptr(), mt.data_ptr(), _pp(lg), _pp(dl), _pp(cells), gt.data_ptr(), ws.data_ptr(), n,
                         loss.data_ptr(), _pp(gl) if grads else None, _pp(gd) if grads else None, _stream())
    assert rc == 0, lib.gsr_last_error()
    return dict(loss=loss, grad_logits=torch.cat([g.reshape(-1) for g in gl]), grad_deltas=torch.cat([g.reshape(-1) for g in gd]))


@pytest.mark.parametrize("c", RC.CASES, ids=lambda c: c.id)
def test_labels_equal_the_oracle_and_the_host_build(RO, host, c):
    ref = RC.reference(c.id)
    assert RC.margins_ok(ref)
    got = {k: v.cpu().numpy() for k, v in _raw_label(RO, c, ref).items()}
    hb = RC.host_labels(host, c, ref)
    for k in ("pre", "labels", "matched", "counts"):
        assert not (got[k] == RC.ISENT).any(), (c.id, k)                          # every element written
        assert np.array_equal(got[k], ref["lab"][k]), (c.id, k, np.nonzero(got[k] != ref["lab"][k]))
        assert np.array_equal(got[k], hb[k]), (c.id, k)


@pytest.mark.parametrize("c", RC.CASES, ids=lambda c: c.id)
def test_loss_and_gradients_within_the_bound(RO, c):
    ref = RC.reference(c.id)
    assert RC.margins_ok(ref)
    got = _raw_loss(RO, c, ref)
    assert not (got["grad_logits"] == RC.FSENT).any() and not (got["grad_deltas"] == RC.FSENT).any() and not (got["loss"] == RC.FSENT).any()
    fails = RC.check_losses(c, ref, got, "gpu")
    assert not fails, fails
    # zero for every anchor that is not sampled, and in the four delta channels of an anchor that is not positive
    x_flat, d_flat = RC.flat_head(c, _levels_of(c, got["grad_logits"], 1), _levels_of(c, got["grad_deltas"], 4))
    labels = _t(ref["lab"]["labels"])
    assert (x_flat[labels < 0] == 0).all() and (d_flat[labels != 1] == 0).all()
    if c.poison == "unsampled":
        assert bool(torch.isfinite(got["loss"]).all() and torch.isfinite(got["grad_logits"]).all() and torch.isfinite(got["grad_deltas"]).all())
    if c.id == "none-present":
        assert float(got["loss"][2]) == 0.0
    assert _bits(_raw_loss(RO, c, ref, grads=False)["loss"]) == _bits(got["loss"])  # the loss bits do not depend on the gradients


def _levels_of(c, flat, k):
    """the flat concatenation of the levels' gradients -> per-level tensors [B,kA,Hf,Wf]"""
    out, o = [], 0
    for l in c.levels:
        n = c.B * k * len(l.cells) * l.hf * l.wf
        out.append(flat[o:o + n].reshape(c.B, k * len(l.cells), l.hf, l.wf))
        o += n
    return out


@pytest.mark.parametrize("cid", ["five-levels", "quota-256-128", "r69120"])
def test_same_bits_again_and_on_a_side_stream(RO, cid):
    c, ref = RC.BY_ID[cid], RC.reference(cid)

    def run():
        lab = _raw_label(RO, c, ref)
        out = _raw_loss(RO, c, ref, labels=lab["labels"], matched=lab["matched"])
        return [_bits(lab[k]) for k in ("pre", "labels", "matched", "counts")] + [_bits(out[k]) for k in RC.COMPARED]

    first, second = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert first == second == third


def test_levels_together_equal_the_same_anchors_as_one_level(RO):
    """The rows of a one-level case dealt to two levels (rpnloss_cases.split_rows: the second level's shift and cell anchors put
    its anchors where the first level's lower rows were): the same anchors in the same flat order, so every integer output and
    every gradient element has the same bits; the loss is the same sum over other blocks."""
    one, ref = RC.BY_ID["as-one"], RC.reference("as-one")
    two, ref2 = RC.split_rows(one, ref, 7)
    assert np.array_equal(RC.anchors(one, np.float32), RC.anchors(two, np.float32))
    whole, parts = _raw_label(RO, one, ref), _raw_label(RO, two, ref2)
    assert all(_bits(whole[k]) == _bits(parts[k]) for k in ("pre", "labels", "matched", "counts"))
    lw, lp = _raw_loss(RO, one, ref), _raw_loss(RO, two, ref2)
    h0 = two.levels[0].hf
    for k, ch in (("grad_logits", 1), ("grad_deltas", 4)):
        a, (p0, p1) = _levels_of(one, lw[k], ch)[0], _levels_of(two, lp[k], ch)
        assert _bits(a[:, :, :h0].contiguous()) == _bits(p0) and _bits(a[:, :, h0:].contiguous()) == _bits(p1)
    assert torch.allclose(lw["loss"], lp["loss"], rtol=1e-6, atol=0)


def test_rpn_loss_class_equals_the_raw_entries_and_autograd_scales(RO):
    from gsplat_attack.proposals import RpnLoss
    c, ref = RC.BY_ID["two-levels"], RC.reference("two-levels")
    inp = ref["inp"]
    raw_lab = _raw_label(RO, c, ref)
    raw = _raw_loss(RO, c, ref, labels=raw_lab["labels"], matched=raw_lab["matched"])
    rl = RpnLoss([(torch.tensor(np.asarray(l.cells, np.float32)), l.stride, l.offset) for l in c.levels], batch_per_image=c.batch,
                 positive_fraction=c.quota / c.batch, beta=c.beta, cls=c.w[0], loc=c.w[1], seed=c.seed)
    lg = [_t(x).requires_grad_(True) for x in inp["logits"]]
    dl = [_t(d).requires_grad_(True) for d in inp["deltas"]]
    lab = rl.labels(lg, _t(inp["gt"]), _t(inp["cls"]), want_pre=True)
    assert all(_bits(a) == _bits(raw_lab[k]) for a, k in ((lab.labels, "labels"), (lab.matched, "matched"), (lab.counts, "counts"), (lab.prelabels, "pre")))
    total, terms = rl.loss(lg, dl, _t(inp["gt"]), _t(inp["cls"]))
    assert _bits(total) == _bits(raw["loss"][0]) and _bits(terms) == _bits(raw["loss"][1:]) and not terms.requires_grad
    (total * 2.5).backward()
    got = torch.cat([t.grad.reshape(-1) for t in lg]), torch.cat([t.grad.reshape(-1) for t in dl])
    assert torch.equal(got[0], raw["grad_logits"] * 2.5) and torch.equal(got[1], raw["grad_deltas"] * 2.5)
    # float16 inputs: converted on the way in, the gradients cast back
    lg16 = [_t(x).half().requires_grad_(True) for x in inp["logits"]]
    dl16 = [_t(d).half().requires_grad_(True) for d in inp["deltas"]]
    t16, _ = rl.loss(lg16, dl16, _t(inp["gt"]), _t(inp["cls"]))
    t16.backward()
    assert all(t.grad.dtype == torch.float16 and t.grad.shape == t.shape for t in lg16 + dl16) and bool(torch.isfinite(t16))


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _chain(with_rpn_loss):
    import test_gpu_rpn as TR
    from gsplat_attack.proposals import RpnLoss, cell_anchors
    from gsplat_attack.roi_detector import ProposalSampler, RoIHeadLoss, make_roi_loss_fn
    net = TR.Net().to(DEV)
    sampler = ProposalSampler(TR.E_NC, per_image=8, positive_fraction=0.25, seed=5)
    kw = {}
    if with_rpn_loss is not False:
        kw["rpn_loss"] = None if with_rpn_loss is None else RpnLoss([(cell_anchors((24,), (0.5, 1.0, 2.0)), TR.E_STRIDE, 0.0)],
                                                                    batch_per_image=16, positive_fraction=0.5, seed=11)
    fn = make_roi_loss_fn(net.backbone, TR._proposer(net), net.box_head, None, sampler, RoIHeadLoss(TR.E_NC, cls=1.0, box=1.0), TR.GT, TR.TARGET,
                          output_size=(TR.E_P, TR.E_P), spatial_scale=1.0 / TR.E_STRIDE, **kw)
    return fn, net, TR


@pytest.fixture
def deterministic_conv():
    """torch's own convolution backward picks, by the process's history, between solvers of which some sum a weight gradient
    with atomics: two identical nets' conv.weight.grad then differ in the last bit, whatever this library does.  The test
    below compares such gradients bit for bit, so it asks torch for its deterministic solvers; the flag is put back."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def test_pgd_attack_with_the_rpn_losses_repeats_and_reaches_the_head(deterministic_conv):
    from gsplat_attack.attack import pgd_attack
    from gsplat_attack.renderer import PipelineParams, render_batch
    hists, params = [], []
    for _ in range(2):
        loss_fn, net, TR = _chain(True)
        model, cams, bg = TR._scene()
        hists.append(pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=True, loss_fn=loss_fn))
        params.append([model.named_parameters()[n].detach().clone() for n in TR.PARAMS])
    torch.cuda.synchronize()
    for h in hists:
        assert len(h) == 2 and all(np.isfinite(v) for v in h) and h[0] != h[1]
    assert hists[0] == hists[1]
    assert all(torch.equal(a, b) for a, b in zip(params[0], params[1]))
    # a gradient at the RPN head's weights (without rpn_loss the head runs under no_grad: none), and rpn_loss=None as before
    model, cams, bg = TR._scene()
    with torch.no_grad():
        renders = render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"]
    loss_fn, net, _ = _chain(True)
    loss_fn(renders, idx=[0, 1]).backward()
    assert net.rpn.weight.grad is not None and float(net.rpn.weight.grad.abs().max()) > 0
    fn_none, net_none, _ = _chain(None)
    fn_omit, net_omit, _ = _chain(False)
    a, b = fn_none(renders, idx=[0, 1]), fn_omit(renders, idx=[0, 1])
    assert _bits(a) == _bits(b)
    a.backward()
    b.backward()
    assert net_none.rpn.weight.grad is None and net_omit.rpn.weight.grad is None
    assert torch.equal(net_none.conv.weight.grad, net_omit.conv.weight.grad)
    assert float(loss_fn(renders, idx=[0, 1]).detach()) != float(a.detach())                      # the RPN losses are in the total

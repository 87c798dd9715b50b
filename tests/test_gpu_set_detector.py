"""The set-prediction detector stage on the device: every case of tests/setdet_cases.py against the float64 PyTorch oracle
(match and tgt integer-equal to the oracle and to the host build; loss[4], grad_logits and grad_boxes within 4 x the
float32 oracle's own error, floor 2^-22, never above 1e-3), the same bits on every call, on a side stream and with or
without the gradients and the optional outputs, every gradient element written, the autograd function, the output stage
followed by gsr_det_verdict against the host restatement, and the stage behind a small torch head as pgd_attack's loss_fn:
render -> head -> loss -> backward to the Gaussian parameters, bit for bit repeatable.  What the kernels add to the scalar
source has cases of its own (setdet_cases: Q and C + 1 at the wave and workgroup widths, the stride loops' second trips,
every maximum at once) and hand-made inputs: exact ties against the serial match, the backward at its kinks, the output
stage at exact scores and at its limits, sentinel words around every output of the C entries, and non-finite inputs."""
import ctypes

import numpy as np
import pytest
import torch

import detect_cases as DT
import setdet_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def SO():
    import diff_gaussian_rasterization as D
    from diff_gaussian_rasterization import setdet_ops
    D._load()
    assert setdet_ops.available()
    return setdet_ops


@pytest.fixture(scope="module")
def host():
    return SC.host_lib()


def _spec(SO, **kw):
    return SO.SetDetSpec(img_w=SC.FRAME[0], img_h=SC.FRAME[1], **kw)


def _dev(ref):
    return tuple(torch.tensor(np.array(ref[k])).to(DEV) for k in ("logits", "boxes", "gt_boxes", "gt_cls"))


def _check(c, got, ref, who):
    """match and tgt integer-equal, loss / grad_logits / grad_boxes within the bound; prints each figure first."""
    o = ref["o64"]
    assert torch.equal(got["match"].cpu(), o["match"]), f"{who} {c.id}: match differs"
    assert torch.equal(got["tgt"].cpu(), o["tgt"]), f"{who} {c.id}: tgt differs"
    fails = []
    for k in SC.COMPARED:
        e, y = SC.err(got[k], o[k]), ref["yard"][k]
        b = SC.bound(y)
        print(f"{who} {c.id} {k}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {b:.3e}")
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, f"{who} {c.id}: {fails}"


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _raw_call(SO, spec, x, bx, gb, gc, gl, gbx, match=None, tgt=None):
    """The C entry on caller buffers (the binding allocates its own): gl / gbx (and match / tgt) arrive pre-filled."""
    B, Q, n1 = x.shape
    cs = SO.c_spec(spec, B, Q, n1 - 1, gb.shape[1])
    ws = torch.empty(((SO.workspace_bytes(cs) + 15) // 16 * 2,), dtype=torch.int64, device=DEV)
    loss = torch.empty(4, dtype=torch.float32, device=DEV)
    lib = SO._lib()
    rc = lib.gsr_setdet_loss(ctypes.byref(cs), x.data_ptr(), bx.data_ptr(), gb.data_ptr(), gc.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                             loss.data_ptr(), gl.data_ptr(), gbx.data_ptr(), None if match is None else match.data_ptr(),
                             None if tgt is None else tgt.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.gsr_last_error()
    return loss


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_kernels_against_the_oracle_and_repeat(SO, host, c):
    ref = SC.reference(c)
    assert SC.margins_ok(ref) and ref["yard_match_equal"]
    x, bx, gb, gc = _dev(ref)
    spec = _spec(SO)
    loss, gl, gbx, match, tgt = SO.run(x, bx, gb, gc, spec)
    torch.cuda.synchronize()
    assert torch.isfinite(gl).all() and torch.isfinite(gbx).all() and torch.isfinite(loss).all()
    _check(c, dict(match=match, tgt=tgt, loss=loss, grad_logits=gl, grad_boxes=gbx), ref, "device")
    # ... and integer-equal to the host build of the same source
    h = SC.host_run(host, ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"], want_grad=False)
    assert np.array_equal(match.cpu().numpy(), h["match"]) and np.array_equal(tgt.cpu().numpy(), h["tgt"])
    # unmatched queries: zero box gradients
    assert (gbx[tgt < 0] == 0).all()
    # the same call again, and once on a side stream: identical bits
    again = SO.run(x, bx, gb, gc, spec)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = SO.run(x, bx, gb, gc, spec)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b2, b3 in zip((loss, gl, gbx, match, tgt), again, other):
        assert _bits(a) == _bits(b2) and _bits(a) == _bits(b3)
    # no gradients and no match / tgt outputs: the same loss bits; the gradients without the optional outputs: the same bits
    bare = SO.run(x, bx, gb, gc, spec, want_grad=False, want_matching=False)
    assert bare[1] is None and bare[2] is None and bare[3] is None and bare[4] is None and _bits(bare[0]) == _bits(loss)
    half = SO.run(x, bx, gb, gc, spec, want_grad=True, want_matching=False)
    assert _bits(half[0]) == _bits(loss) and _bits(half[1]) == _bits(gl) and _bits(half[2]) == _bits(gbx)
    only = SO.run(x, bx, gb, gc, spec, want_grad=False, want_matching=True)
    assert _bits(only[0]) == _bits(loss) and _bits(only[3]) == _bits(match) and _bits(only[4]) == _bits(tgt)
    # every gradient element is written: none keeps the sentinel the buffers were filled with
    s_gl, s_gbx = torch.full_like(gl, SENTINEL), torch.full_like(gbx, SENTINEL)
    s_loss = _raw_call(SO, spec, x, bx, gb, gc, s_gl, s_gbx)
    torch.cuda.synchronize()
    assert _bits(s_loss) == _bits(loss) and _bits(s_gl) == _bits(gl) and _bits(s_gbx) == _bits(gbx)
    assert not (s_gl == SENTINEL).any() and not (s_gbx == SENTINEL).any()


def _run_np(SO, inputs, **kw):
    """SO.run on numpy inputs -> dict of numpy outputs (after a synchronise)."""
    dev = tuple(torch.tensor(np.array(a)).to(DEV) for a in inputs)
    loss, gl, gbx, match, tgt = SO.run(*dev, _spec(SO), **kw)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu().numpy(), grad_logits=gl.cpu().numpy(), grad_boxes=gbx.cpu().numpy(), match=match.cpu().numpy(),
                tgt=tgt.cpu().numpy())


@pytest.mark.parametrize("kind", SC.TIE_KINDS)
def test_exact_ties_equal_the_serial_match(SO, host, kind):
    """setdet_cases.tie_inputs: equal candidates meet in the lanes' own scans, in the wave butterfly, in the merge of the four
    waves and across the trips of the stride loop, and the lane-dealt match must return what the serial one does (the host
    build; test_setdet_host_cpu.py holds that to the stated rule): integer-equal match and tgt, one-to-one, the oracle's
    optimum in the oracle's own float64 cost matrix, loss and gradients within the bound with this match frozen."""
    ref = SC.tie_reference(kind)
    assert ref["gap"] > SC.GAP_MATCH
    want = SC.host_run(host, *ref["inputs"], want_grad=False)
    got = _run_np(SO, ref["inputs"])
    SC.check_tie("device", kind, got, want["match"])
    assert np.array_equal(got["tgt"], want["tgt"])
    again = _run_np(SO, ref["inputs"])
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_backward_at_its_kinks(SO, host):
    """setdet_cases.kink_inputs, one image per kink: within the usual bound of the float64 oracle, whose autograd follows the
    contract's conventions there; where every step of the box gradient is exact (KINK_EXACT) the same bits as the host
    build of the same source."""
    inputs = SC.kink_inputs()
    o = SC.oracle(*inputs, want_gap=True)
    assert o["gap_match"] > SC.GAP_MATCH
    got = _run_np(SO, inputs)
    assert np.array_equal(got["match"], o["match"].numpy()) and np.array_equal(got["tgt"], o["tgt"].numpy())
    assert np.isfinite(got["grad_boxes"]).all() and np.isfinite(got["grad_logits"]).all() and np.isfinite(got["loss"]).all()
    SC.check_with_match_frozen("device kinks", got, inputs)
    h = SC.host_run(host, *inputs)
    names = [k[0] for k in SC.KINKS]
    for name in SC.KINK_EXACT:
        b = names.index(name)
        print(f"kink {name}: device {got['grad_boxes'][b, 0].tolist()} host {h['grad_boxes'][b, 0].tolist()}")
        assert got["grad_boxes"][b].tobytes() == h["grad_boxes"][b].tobytes(), name
    assert (got["grad_boxes"][names.index("equal")] == 0).all() and (got["grad_boxes"][:, 1] == 0).all()


def test_postprocess_at_exact_scores_and_limits(SO):
    """The output stage at exact scores (a class tie at 0.5, a score exactly at conf_thr, NaN and -inf logits), at max_det = 1
    on 1024 queries and 1024 on 65, with all and none of 65 queries kept: setdet_cases.exact_score_expectations, what the
    host build is held to as well."""
    def post(x, bx, thr, max_det):
        dets, counts = SO.postprocess(torch.tensor(np.array(x)).to(DEV), torch.tensor(np.array(bx)).to(DEV),
                                      _spec(SO, conf_thr=thr, max_det=max_det))
        torch.cuda.synchronize()
        return dets.cpu().numpy(), counts.cpu().numpy()
    SC.exact_score_expectations(post)


PAD, F_FILL, I_FILL = 256, -12345.0, 0x5A5A5A5A


def _padded(n, dtype):
    """-> (buffer of PAD + n + PAD sentinel words, the address of word PAD)."""
    buf = torch.full((PAD + n + PAD,), F_FILL if dtype == torch.float32 else I_FILL, dtype=dtype, device=DEV)
    return buf, buf.data_ptr() + 4 * PAD


def _pads_untouched(buf, n):
    fill = F_FILL if buf.dtype == torch.float32 else I_FILL
    return bool((buf[:PAD] == fill).all() and (buf[PAD + n:] == fill).all())


def test_nothing_is_written_outside_the_outputs(SO):
    """The C entries on caller buffers with 256 sentinel words on either side of every output, the optional match and tgt
    among them, and behind the workspace: the binding's bits inside, every sentinel outside."""
    B, Q, C, M = 2, 65, 4, 5
    x, bx, gb, gc = (torch.tensor(a).to(DEV) for a in SC.make_inputs(SC.Case("pads", B, Q, C, M)))
    spec = _spec(SO)
    want = SO.run(x, bx, gb, gc, spec)
    sizes = (4, B * Q * (C + 1), B * Q * 4, B * M, B * Q)
    bufs = [_padded(n, torch.float32 if k < 3 else torch.int32) for k, n in enumerate(sizes)]
    cs = SO.c_spec(spec, B, Q, C, M)
    ws_bytes = SO.workspace_bytes(cs)
    assert ws_bytes % 4 == 0
    ws = torch.full((ws_bytes // 4 + PAD,), I_FILL, dtype=torch.int32, device=DEV)
    lib = SO._lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.gsr_setdet_loss(ctypes.byref(cs), x.data_ptr(), bx.data_ptr(), gb.data_ptr(), gc.data_ptr(), ws.data_ptr(), ws_bytes,
                             *[p for _, p in bufs], stream)
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    for (buf, _), n, w in zip(bufs, sizes, want):
        assert _bits(buf[PAD:PAD + n]) == _bits(w.reshape(-1)) and _pads_untouched(buf, n)
    assert (ws[ws_bytes // 4:] == I_FILL).all()
    # without the optional outputs and the gradients: the loss alone, nothing else touched
    for buf, _ in bufs:
        buf.fill_(F_FILL if buf.dtype == torch.float32 else I_FILL)
    rc = lib.gsr_setdet_loss(ctypes.byref(cs), x.data_ptr(), bx.data_ptr(), gb.data_ptr(), gc.data_ptr(), ws.data_ptr(), ws_bytes,
                             bufs[0][1], None, None, None, None, stream)
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    assert _bits(bufs[0][0][PAD:PAD + 4]) == _bits(want[0]) and _pads_untouched(bufs[0][0], 4)
    assert all((buf == (F_FILL if buf.dtype == torch.float32 else I_FILL)).all() for buf, _ in bufs[1:])
    assert (ws[ws_bytes // 4:] == I_FILL).all()
    # the output stage: fewer rows than kept queries, and as many rows as queries
    for max_det in (3, Q):
        pspec = _spec(SO, conf_thr=SC.CONF_THR, max_det=max_det)
        wd, wn = SO.postprocess(x, bx, pspec)
        assert int(wn[:, 1].min()) > 3                                      # max_det = 3 cuts every image's rows
        dets, counts = _padded(B * max_det * 6, torch.float32), _padded(B * 2, torch.int32)
        pcs = SO.c_spec(pspec, B, Q, C, 1)
        rc = lib.gsr_setdet_postprocess(ctypes.byref(pcs), x.data_ptr(), bx.data_ptr(), dets[1], counts[1], stream)
        assert rc == 0, lib.gsr_last_error()
        torch.cuda.synchronize()
        assert _bits(dets[0][PAD:PAD + B * max_det * 6]) == _bits(wd.reshape(-1)) and _pads_untouched(dets[0], B * max_det * 6)
        assert _bits(counts[0][PAD:PAD + B * 2]) == _bits(wn.reshape(-1)) and _pads_untouched(counts[0], B * 2)


def test_other_weights_than_the_defaults(SO):
    """The cost and loss weights reach the kernels: another set of them against the oracle run with the same."""
    c = SC.BY_ID["contested"]
    ref = SC.reference(c)
    x, bx, gb, gc = _dev(ref)
    costs, w, eos = (2.0, 1.0, 3.0), (0.5, 2.0, 4.0), 0.25
    o64 = SC.oracle(ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"], costs=costs, w=w, eos=eos, want_gap=True)
    o32 = SC.oracle(ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"], torch.float32, costs=costs, w=w, eos=eos)
    print(f"other weights: gap_match {o64['gap_match']:.3e}")
    assert o64["gap_match"] > SC.GAP_MATCH and torch.equal(o32["match"], o64["match"])
    assert not torch.equal(o64["match"], ref["o64"]["match"])              # the other cost weights match differently
    spec = _spec(SO, c_class=costs[0], c_l1=costs[1], c_giou=costs[2], w_ce=w[0], w_l1=w[1], w_giou=w[2], eos_coef=eos)
    loss, gl, gbx, match, tgt = SO.run(x, bx, gb, gc, spec)
    other = dict(o64=o64, yard={k: SC.err(o32[k], o64[k]) for k in SC.COMPARED})
    _check(c, dict(match=match, tgt=tgt, loss=loss, grad_logits=gl, grad_boxes=gbx), other, "device, other weights")


def test_autograd_function_under_a_non_unit_upstream_gradient(SO):
    c = SC.BY_ID["ragged"]
    ref = SC.reference(c)
    x0, bx0, gb, gc = _dev(ref)
    spec = _spec(SO)
    x, bx = x0.clone().requires_grad_(True), bx0.clone().requires_grad_(True)
    total, items = SO.setdet_loss(x, bx, gb, gc, spec)
    assert not items.requires_grad and total.requires_grad
    (total * 3.0).backward()
    loss, gl, gbx, _, _ = SO.run(x0, bx0, gb, gc, spec)
    assert _bits(total) == _bits(loss[3]) and _bits(items) == _bits(loss[:3])
    assert torch.equal(x.grad, gl * 3.0) and torch.equal(bx.grad, gbx * 3.0)
    # only the boxes require grad: logits get none
    bx2 = bx0.clone().requires_grad_(True)
    t2, _ = SO.setdet_loss(x0, bx2, gb, gc, spec)
    t2.backward()
    assert torch.equal(bx2.grad, gbx) and x0.grad is None
    with torch.no_grad():
        t3, _ = SO.setdet_loss(x0, bx0, gb, gc, spec)
    assert _bits(t3) == _bits(loss[3]) and not t3.requires_grad


# ---- the output stage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_postprocess_equals_the_host_build_and_the_restatement(SO, host, c):
    """Bit-equal to the host build of the same source except the score, where the device's exp and the host's may round
    differently (within setdet_cases.score_tol); integer-equal in counts, order and classes to the torch restatement of
    detr_detector.py:186-202."""
    ref = SC.reference(c)
    x, bx, _, _ = _dev(ref)
    want, wcounts, gap_score, gap_lead = ref["post"]
    assert gap_score > SC.GAP_SCORE and gap_lead > SC.GAP_LEAD
    dets, counts = SO.postprocess(x, bx, _spec(SO, conf_thr=SC.CONF_THR))
    again = SO.postprocess(x, bx, _spec(SO, conf_thr=SC.CONF_THR))
    torch.cuda.synchronize()
    assert _bits(dets) == _bits(again[0]) and _bits(counts) == _bits(again[1])
    d, n = dets.cpu().numpy(), counts.cpu().numpy()
    hd, hn = SC.host_post(host, ref["logits"], ref["boxes"])
    assert np.array_equal(n, wcounts) and np.array_equal(n, hn)
    assert np.array_equal(d[..., :4], hd[..., :4]) and np.array_equal(d[..., :4], want[..., :4])
    assert np.array_equal(d[..., 5], want[..., 5]) and np.array_equal(d[..., 5], hd[..., 5])
    tol = SC.score_tol(c.C)
    print(f"postprocess {c.id}: score max abs diff to the restatement {np.abs(d[..., 4] - want[..., 4]).max():.3e}, to the host "
          f"build {np.abs(d[..., 4] - hd[..., 4]).max():.3e}, tol {tol:.3e}")
    assert np.abs(d[..., 4] - want[..., 4]).max() <= tol and np.abs(d[..., 4] - hd[..., 4]).max() <= tol
    for b in range(c.B):
        assert (d[b, n[b, 0]:] == 0).all()
    if wcounts[:, 1].max() > 1:                                            # fewer rows than kept queries
        k = int(wcounts[:, 1].max()) - 1
        d2, n2 = SO.postprocess(x, bx, _spec(SO, conf_thr=SC.CONF_THR, max_det=k))
        assert np.array_equal(n2.cpu().numpy()[:, 1], wcounts[:, 1]) and np.array_equal(n2.cpu().numpy()[:, 0], np.minimum(wcounts[:, 1], k))
        assert np.array_equal(d2.cpu().numpy(), d[:, :k])


def test_verdicts_equal_the_host_restatement():
    """SetDetectorOutput.verdicts = gsr_setdet_postprocess + gsr_det_verdict against detr_detector.py:216-243 restated on the
    host (detect_cases.oracle_verdict) over the restated detections: targeted, untargeted, no gt box and no rows."""
    from gsplat_attack.set_detector import SetDetectorOutput
    c = SC.BY_ID["ragged"]
    ref = SC.reference(c)
    x, bx, _, _ = _dev(ref)
    want, wcounts, _, _ = ref["post"]
    rng = np.random.default_rng(31)
    gt = np.zeros((c.B, 4), np.float32)
    picked = []
    for b in range(c.B):                                                   # a jittered copy of one kept detection per image
        r = want[b, rng.integers(0, wcounts[b, 0])]
        picked.append(int(r[5]))
        w, h = r[2] - r[0], r[3] - r[1]
        gt[b] = r[:4] + rng.uniform(-0.1, 0.1, 4) * [w, h, w, h]
    out = SetDetectorOutput(SC.FRAME, conf=SC.CONF_THR)
    combos = [(picked[0], None, True), (picked[1], picked[2], True), (picked[0], picked[1], False), (c.C - 1, picked[2], False)]
    for target, untarget, targeted in combos:
        bits, best, gap = DT.oracle_verdict(want, wcounts, gt, target, untarget, targeted, 0.5)
        assert gap > DT.MARGIN
        flags, gbest = out.verdicts(x, bx, torch.tensor(gt), target, untarget, targeted)
        assert flags.cpu().tolist() == bits.tolist(), (target, untarget, targeted)
        assert np.array_equal(gbest.cpu().numpy()[:, 2:], best[:, 2:].astype(np.float32))     # class and row of the best
        assert np.abs(gbest.cpu().numpy()[:, 0] - best[:, 0]).max() < 1e-5
    assert any(DT.oracle_verdict(want, wcounts, gt, t, u, k, 0.5)[0][0] & 1 for t, u, k in combos)
    # no gt box: None, and a NaN row in one image
    for g in (None, np.where(np.arange(c.B)[:, None] == 1, np.nan, gt).astype(np.float32)):
        bits, best, _ = DT.oracle_verdict(want, wcounts, g, picked[0], picked[1], True, 0.5)
        flags, _ = out.verdicts(x, bx, None if g is None else torch.tensor(g), picked[0], picked[1], True)
        assert flags.cpu().tolist() == bits.tolist()
    # no rows: nothing exceeds the threshold
    none = SetDetectorOutput(SC.FRAME, conf=1.5)
    dets, counts = none.detect(x, bx)
    assert (counts == 0).all() and (dets == 0).all()
    for targeted in (True, False):
        bits, _, _ = DT.oracle_verdict(np.zeros_like(want), np.zeros_like(wcounts), gt, picked[0], picked[1], targeted, 0.5)
        flags, gbest = none.verdicts(x, bx, torch.tensor(gt), picked[0], picked[1], targeted)
        assert flags.cpu().tolist() == bits.tolist() and (gbest == -1).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------
NC, PER_CELL, CELL = 3, 2, 16      # classes; queries per cell; a 64 x 64 render in 4 x 4 cells: 32 queries
GT = torch.tensor([[10.3, 12.6, 52.2, 49.7], [14.4, 7.7, 56.3, 54.1]])   # per view, render frame
TARGET = 1


class Head(torch.nn.Module):
    """One strided convolution of the render -> Q = 32 queries with NC + 1 logits and a sigmoid box each; fixed-seed weights."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(23)
        self.conv = torch.nn.Conv2d(3, PER_CELL * (NC + 5), CELL, stride=CELL)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.05)
            self.conv.bias.copy_(torch.randn(self.conv.bias.shape, generator=g) * 0.5)

    def forward(self, x):
        f = self.conv(x)                                                   # [B, PER_CELL * (NC + 5), 4, 4]
        B = f.shape[0]
        f = f.reshape(B, PER_CELL, NC + 5, -1).permute(0, 1, 3, 2).reshape(B, -1, NC + 5)
        return {"pred_logits": f[..., :NC + 1], "pred_boxes": torch.sigmoid(f[..., NC + 1:])}


def _scene():
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), width=64, height=64, n_views=2)
    return model, cams, torch.tensor([0.1, 0.2, 0.3], device=DEV)


def _loss_fn():
    from gsplat_attack.set_detector import SetDetectorLoss, make_set_loss_fn
    head = Head().to(DEV)
    return make_set_loss_fn(head, None, SetDetectorLoss(NC, (64, 64)), GT, TARGET), head


PARAMS = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")


def test_loss_fn_gradients_reach_the_gaussians_and_repeat():
    from gsplat_attack.renderer import PipelineParams, render_batch
    model, cams, bg = _scene()
    loss_fn, head = _loss_fn()
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
    # the loss the stage returned is the oracle's for the head's output on these renders
    with torch.no_grad():
        out = head(render_batch(cams, model, PipelineParams(skip_objects=True), bg)["render"])
    lg, bx = out["pred_logits"].cpu().numpy(), out["pred_boxes"].cpu().numpy()
    cls = np.full((2, 1), TARGET, np.int32)
    o64 = SC.oracle(lg, bx, GT[:, None, :].numpy(), cls, frame=(64.0, 64.0), want_gap=True)
    o32 = SC.oracle(lg, bx, GT[:, None, :].numpy(), cls, torch.float32, frame=(64.0, 64.0))
    e, y = SC.err(runs[0][0], o64["loss"][3]), SC.err(o32["loss"][3], o64["loss"][3])
    print(f"end to end: gap_match {o64['gap_match']:.3e} total err {e:.3e} yardstick {y:.3e} bound {SC.bound(y):.3e}")
    assert o64["gap_match"] > SC.GAP_MATCH and e <= SC.bound(y)


def test_pgd_attack_with_the_set_loss_repeats():
    from gsplat_attack.attack import pgd_attack
    hists, params = [], []
    for batch_loss in (True, True, False, False):
        model, cams, bg = _scene()
        loss_fn, _ = _loss_fn()
        hists.append(pgd_attack(model, cams, iters=2, groups=("color",), bg=bg, batch_loss=batch_loss, loss_fn=loss_fn))
        params.append([model.named_parameters()[n].detach().clone() for n in PARAMS])
    torch.cuda.synchronize()
    for h in hists:
        assert len(h) == 2 and all(np.isfinite(v) for v in h) and h[0] != h[1]     # the step moved the loss
    assert hists[0] == hists[1] and hists[2] == hists[3]
    for i, j in ((0, 1), (2, 3)):
        assert all(torch.equal(a, b) for a, b in zip(params[i], params[j]))
    fresh = _scene()[0].named_parameters()
    assert not all(torch.equal(a, fresh[n].detach()) for a, n in zip(params[0], PARAMS))       # the attack moved the parameters


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.NONFINITE_CASES, ids=lambda c: c.id)
def test_non_finite_inputs_stay_in_range_and_in_their_image(SO, c):
    """NaN and +-inf in the logits and boxes of image 1 of three (setdet_cases.poisoned_inputs, shares 0.05, 0.5 and 1 of the
    elements): the poisoned image's floats are unspecified, but every call returns, every index is in range, the match is
    one-to-one over the present rows with tgt its inverse, every gradient element is written, the output stage's counts lie
    in 0..Q, and images 0 and 2 keep the clean run's bits.

    Why the kernels end and stay in range whatever the floats are (read from the source, not found by running):
      * every loop of the five kernels is bounded by B, Q, C, M or a constant: the stride loops by Q, B, n or nblocks, the
        match's row loop by M, its pass loop by `it <= M`, the path flip by `it <= M`;
      * in k_setdet_match every value that steers a barrier or a break is the same in all lanes: i, present(s_cls[..]) and
        s_p[j0] are read from LDS behind a barrier, j0 follows j1, and (delta, j1) are recomputed by every thread from
        s_bv / s_bj behind a barrier (only lane 0 of a wave writes them, so lanes whose butterflies disagree over a NaN do
        not matter); a delta that is not below +inf -- NaN included -- takes the lowest unmarked column with delta = 0;
      * every index is an integer the algorithm made (s_p in 0..M, s_way in 0..Q, bj in {-1, 1..Q} and only ever an unmarked
        column, so each pass marks a new one) or is clamped before use (tg < M, i <= M, present(tc), bc < C);
      * the normalisers are integers (matched rows, B * Q) and every present row is matched either way, so nothing of image
        1 reaches the other images' terms."""
    logits, boxes, gtb, gtc = SC.make_inputs(c)
    gb, gc = torch.tensor(gtb).to(DEV), torch.tensor(gtc).to(DEV)
    spec = _spec(SO)
    clean = _run_np(SO, (logits, boxes, gtb, gtc))
    for frac in SC.NONFINITE_FRACS:
        x, bx = (torch.tensor(a).to(DEV) for a in SC.poisoned_inputs(c, frac))
        gl, gbx = torch.full_like(x, SENTINEL), torch.full_like(bx, SENTINEL)
        match = torch.full((c.B, c.M), -9, dtype=torch.int32, device=DEV)
        tgt = torch.full((c.B, c.Q), -9, dtype=torch.int32, device=DEV)
        _raw_call(SO, spec, x, bx, gb, gc, gl, gbx, match, tgt)
        _, counts = SO.postprocess(x, bx, _spec(SO, conf_thr=SC.CONF_THR))
        torch.cuda.synchronize()                                           # raises on any HIP error
        assert not (gl == SENTINEL).any() and not (gbx == SENTINEL).any()
        got = dict(match=match.cpu().numpy(), tgt=tgt.cpu().numpy(), grad_logits=gl.cpu().numpy(), grad_boxes=gbx.cpu().numpy())
        SC.check_poisoned(f"device {c.id} {frac}", c, got, clean, gtc, counts.cpu().numpy())

"""The two-stage detector stage on the device: every case of tests/rcnn_cases.py against the float64 PyTorch oracle (the
sampler's idx, labels, gt_row, counts and the output stage's counts, kept classes and kept order integer-equal to the oracle
and to the host build; pooled, grad_features, loss, grad_scores and grad_deltas within 4 x the float32 oracle's own error,
floor 2^-22, never above 1e-3), the margins asserted in front of every comparison, every output element written and nothing
beside it (every C entry runs on sentinel-filled outputs between guard words, the workspaces with a guard behind), the same
bits on every call and on a side stream, `accumulate`, an image without RoIs, what the margins exclude against rows written
out by hand (a sample exactly on the map's edge, an IoU exactly at fg_iou, identical gt rows, a score exactly at conf_thr, a
class tie, non-finite logits), the guards on labels and gt_row, the autograd functions, verdicts against a host restatement,
and the stage behind a small torch backbone and box head as pgd_attack's loss_fn, bit for bit repeatable.  DESIGN.md has the
measured ratios and the mutants each group of cases was checked against."""
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


# ---- caller buffers between guard words -----------------------------------------------------------------------------------
GUARD = 256                # 4-byte words on either side of an output: 1 KiB, so the view between them keeps its alignment
PATTERN = 0x5A5A5A5A
WS_GUARD = 1024            # bytes behind a workspace


class _Guarded:
    """An output tensor of `shape`, filled with `fill`, between two runs of guard words."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.store = torch.full((GUARD + n + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.n = n
        self.t = self.store[GUARD:GUARD + n].view(dtype).view(shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.store[:GUARD] == PATTERN).all() and (self.store[GUARD + self.n:] == PATTERN).all())


def _guarded_ws(nbytes):
    ws = torch.full((nbytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    return ws


def _unharmed(bufs, ws=None, nbytes=0):
    """After the call: no guard word around any output (or behind the workspace) was written."""
    torch.cuda.synchronize()
    for k, g in bufs.items():
        assert g.intact(), f"a store outside {k}"
    if ws is not None:
        assert (ws[nbytes:] == 0xA5).all(), "a store behind the workspace"
    return {k: g.t for k, g in bufs.items()}


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def _raw_sample(RO, c, seed, inputs=None):
    """The C entry on sentinel-filled caller buffers between guard words."""
    prop, gt, cls, n_prop = (_t(a) for a in (RC.sample_inputs(c) if inputs is None else inputs))
    cs = RO.c_spec(RO.RcnnSpec(S=c.S, max_pos=c.max_pos, append_gt=c.append_gt, seed=seed, fg_iou=RC.FG_IOU), B=c.B, R=c.R, M=c.M, C=RC.NC)
    bufs = dict(idx=_Guarded((c.B, c.S), torch.int32, ISENT), rois=_Guarded((c.B, c.S, 4), torch.float32, SENTINEL),
                labels=_Guarded((c.B, c.S), torch.int32, ISENT), gt_row=_Guarded((c.B, c.S), torch.int32, ISENT),
                counts=_Guarded((c.B, 2), torch.int32, ISENT))
    out = {k: g.t for k, g in bufs.items()}
    lib = RO._lib()
    rc = lib.gsr_rcnn_sample(ctypes.byref(cs), prop.data_ptr(), None if n_prop is None else n_prop.data_ptr(), gt.data_ptr(),
                             cls.data_ptr(), out["idx"].data_ptr(), out["rois"].data_ptr(), out["labels"].data_ptr(),
                             out["gt_row"].data_ptr(), out["counts"].data_ptr(), _stream())
    assert rc == 0, lib.gsr_last_error()
    return _unharmed(bufs)


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


def test_sampler_exact_decisions_by_hand(RO, host):
    """An IoU of exactly fg_iou is foreground, of identical present rows the lowest is the match, an absent row in front of them
    is skipped: the rows written out by hand in rcnn_cases.sample_exact_inputs, and the host build's bits."""
    c, inputs, want = RC.sample_exact_inputs()
    got, h = _raw_sample(RO, c, c.seed, inputs=inputs), RC.host_sample(host, c, inputs=inputs)
    for k, w in want.items():
        assert np.array_equal(got[k].cpu().numpy(), w) and np.array_equal(h[k], w), k
    assert _bits(got["rois"]) == h["rois"].tobytes() and not (got["rois"] == SENTINEL).any()


# ---- RoIAlign -------------------------------------------------------------------------------------------------------------------
def _roi_raw(RO, c, fill=SENTINEL, accumulate=False, gf=None, inputs=None):
    """The two C entries on caller buffers between guard words (grad_features too, unless the caller brings its own)."""
    feat, gp, rois, n_roi = (_t(a) for a in (RC.roi_case_inputs(c) if inputs is None else inputs))
    cs = RO.c_spec(RO.RcnnSpec(PH=c.PH, PW=c.PW, spatial_scale=c.scale, sampling_ratio=c.ratio), B=feat.shape[0], Cf=c.Cf, Hf=c.Hf, Wf=c.Wf,
                   S=rois.shape[1])
    bufs = dict(pooled=_Guarded(tuple(gp.shape), torch.float32, fill))
    if gf is None:
        bufs["grad_features"] = _Guarded(tuple(feat.shape), torch.float32, fill)
        gf = bufs["grad_features"].t
    pooled = bufs["pooled"].t
    lib = RO._lib()
    assert lib.gsr_roi_align(ctypes.byref(cs), feat.data_ptr(), rois.data_ptr(), n_roi.data_ptr(), 2, pooled.data_ptr(), _stream()) == 0, \
        lib.gsr_last_error()
    assert lib.gsr_roi_align_backward(ctypes.byref(cs), rois.data_ptr(), n_roi.data_ptr(), 2, gp.data_ptr(), gf.data_ptr(),
                                      1 if accumulate else 0, _stream()) == 0, lib.gsr_last_error()
    _unharmed(bufs)
    return dict(pooled=pooled, grad_features=gf)


@pytest.mark.parametrize("c", RC.ROI_CASES, ids=lambda c: c.id)
def test_roi_align_and_its_backward_match_the_oracle(RO, c):
    ref = RC.roi_reference(c)
    assert RC.roi_margins_ok(ref)
    got = _roi_raw(RO, c)
    for k in ("pooled", "grad_features"):
        assert not (got[k] == SENTINEL).any() and torch.isfinite(got[k]).all(), f"{c.id}: {k} holds unwritten elements"
    _check("device", c.id, got, ref, ("pooled", "grad_features"))
    for b, s in RC.roi_dead_rows(c):                                       # beyond the count, or not finite
        assert (got["pooled"][b, s] == 0).all(), (b, s)
    if c.table == "base":
        assert (got["pooled"][0, 7] == 0).all() and (got["pooled"][1, 7:] == 0).all()


@pytest.mark.parametrize("cid", ["wide-zero-c33-r0", "wide-zero-c3-r2", "s1024"])
def test_roi_backward_of_an_image_without_rois(RO, cid):
    """An image whose count is 0: its grad_features are written as zeros, and under `accumulate` they keep the base's bits
    (as do all elements the other image's RoIs do not reach)."""
    c = next(k for k in RC.ROI_CASES if k.id == cid)
    first = _roi_raw(RO, c)
    assert (first["grad_features"][1] == 0).all() and float(first["grad_features"][0].abs().max()) > 0
    assert (first["pooled"][1] == 0).all()
    base = torch.arange(first["grad_features"].numel(), dtype=torch.float32, device=DEV).reshape(first["grad_features"].shape) * 0.25 + 1.0
    acc = _roi_raw(RO, c, accumulate=True, gf=base.clone())
    assert _bits(acc["grad_features"][1]) == _bits(base[1])
    assert torch.equal(acc["grad_features"], base + first["grad_features"])


def test_roi_exact_edges_by_hand(RO, host):
    """A sample at exactly -1 or exactly n reads the border cell with weight 1, the next position further out reads 0; the
    backward puts all of g on that one cell or on none.  The values written out by hand in rcnn_cases.roi_edge_inputs, and the
    host build's bits."""
    c, inputs, pooled, gf, _ = RC.roi_edge_inputs()
    got, h = _roi_raw(RO, c, inputs=inputs), RC.host_roi(host, c, inputs=inputs)
    assert np.array_equal(got["pooled"].cpu().numpy()[0, :, :, 0, 0], pooled) and _bits(got["pooled"]) == h["pooled"].tobytes()
    assert np.array_equal(got["grad_features"].cpu().numpy()[0], gf) and _bits(got["grad_features"]) == h["grad_features"].tobytes()


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


def _loss_raw(RO, c, with_grads=True, inputs=None):
    """The C entry on caller buffers between guard words, the workspace of exactly gsr_rcnn_workspace_bytes with a guard behind."""
    i = RC.loss_inputs(c) if inputs is None else inputs
    x, d, r, lb, gr, gb = (_t(i[k]) for k in ("scores", "deltas", "rois", "labels", "gt_row", "gt_boxes"))
    cs = RO.c_spec(_loss_spec(RO, c), B=c.B, M=c.M, C=c.C, S=c.S)
    cs.R, cs.max_det = 0, 0                                              # the workspace of the loss alone
    nbytes = RO.workspace_bytes(cs)
    ws = _guarded_ws(nbytes)
    bufs = dict(loss=_Guarded((3,), torch.float32, SENTINEL))
    if with_grads:
        bufs.update(grad_scores=_Guarded(tuple(x.shape), torch.float32, SENTINEL), grad_deltas=_Guarded(tuple(d.shape), torch.float32, SENTINEL))
    gs, gd = (bufs["grad_scores"].t, bufs["grad_deltas"].t) if with_grads else (None, None)
    lib = RO._lib()
    rc = lib.gsr_rcnn_loss(ctypes.byref(cs), x.data_ptr(), d.data_ptr(), r.data_ptr(), lb.data_ptr(), gr.data_ptr(), gb.data_ptr(),
                           ws.data_ptr(), nbytes, bufs["loss"].t.data_ptr(), gs.data_ptr() if with_grads else None,
                           gd.data_ptr() if with_grads else None, _stream())
    assert rc == 0, lib.gsr_last_error()
    _unharmed(bufs, ws, nbytes)
    return dict(loss=bufs["loss"].t, grad_scores=gs, grad_deltas=gd)


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


def test_loss_guards_on_labels_and_rows(RO, host):
    """A label above C counts as -1: C + 1, 2^31 - 1 and -7 give the bits of -1 in all three outputs.  A foreground row whose
    gt_row is M, M + 100 or -3 keeps its cross-entropy term and gradient, adds nothing to the box term and gets a zero
    grad_deltas row; everything stays finite and within the bound of the oracle (whose fg has `gt_row < M`)."""
    c, base, bad_lb, clean_lb, bad_gr, rows = RC.loss_guard_inputs()
    a, b_ = _loss_raw(RO, c, inputs=bad_lb), _loss_raw(RO, c, inputs=clean_lb)
    for k in RC.LOSS_COMPARED:
        assert _bits(a[k]) == _bits(b_[k]) and torch.isfinite(a[k]).all() and not (a[k] == SENTINEL).any(), k
    _check("device", "clean-labels", b_, RC.loss_reference_of(c, clean_lb), RC.LOSS_COMPARED)
    ref, g, g0 = RC.loss_reference_of(c, bad_gr), _loss_raw(RO, c, inputs=bad_gr), _loss_raw(RO, c)
    _check("device", "bad-rows", g, ref, RC.LOSS_COMPARED)
    for k in RC.LOSS_COMPARED:
        assert torch.isfinite(g[k]).all() and not (g[k] == SENTINEL).any(), k
    assert _bits(g["loss"][0]) == _bits(g0["loss"][0]) and float(g["loss"][1]) < float(g0["loss"][1])
    assert _bits(g["grad_scores"]) == _bits(g0["grad_scores"])
    for b, s in rows:
        assert (g["grad_deltas"][b, s] == 0).all() and float(g0["grad_deltas"][b, s].abs().max()) > 0
    h = RC.host_loss(host, c, inputs=bad_gr)
    assert (h["grad_deltas"] == 0).tobytes() == (g["grad_deltas"].cpu().numpy() == 0).tobytes()       # the same zero pattern


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


def _post_raw(RO, c, inputs=None):
    """gsr_rcnn_postprocess itself: dets and counts sentinel-filled between guard words, the workspace of exactly
    gsr_rcnn_workspace_bytes, filled with 0xA5, with a guard behind."""
    scores, deltas, prop, n_prop = (_t(a) for a in (RC.post_inputs(c) if inputs is None else inputs))
    Bn, R, C = scores.shape[0], scores.shape[1], scores.shape[2] - 1
    spec = RO.RcnnSpec(conf_thr=c.conf, iou_thr=RC.IOU_THR, max_det=c.max_det, img_w=RC.FRAME[0], img_h=RC.FRAME[1], class_agnostic=c.agnostic)
    cs = RO.c_spec(spec, B=Bn, R=R, C=C, S=0)
    nbytes = RO.workspace_bytes(cs)
    ws = _guarded_ws(nbytes)
    bufs = dict(dets=_Guarded((Bn, c.max_det, 6), torch.float32, SENTINEL), counts=_Guarded((Bn, 2), torch.int32, ISENT))
    lib = RO._lib()
    rc = lib.gsr_rcnn_postprocess(ctypes.byref(cs), scores.data_ptr(), deltas.data_ptr(), prop.data_ptr(), n_prop.data_ptr(), ws.data_ptr(),
                                  nbytes, bufs["dets"].t.data_ptr(), bufs["counts"].t.data_ptr(), _stream())
    assert rc == 0, lib.gsr_last_error()
    out = _unharmed(bufs, ws, nbytes)
    assert not (out["dets"] == SENTINEL).any() and not (out["counts"] == ISENT).any(), f"{c.id}: unwritten elements"
    return out["dets"], out["counts"]


@pytest.mark.parametrize("c", RC.POST_CASES, ids=lambda c: c.id)
def test_output_stage_equals_the_oracle_and_the_host_build(RO, host, c):
    o, h = RC.post_reference(c), RC.host_post(host, c)
    assert RC.post_margins_ok(o)
    scores, deltas, prop, n_prop = (_t(a) for a in RC.post_inputs(c))
    dets, counts = _output(c).detect(scores, deltas, prop, n_prop=n_prop)
    dets2, counts2 = _post_raw(RO, c)
    assert _bits(dets) == _bits(dets2) and _bits(counts) == _bits(counts2)
    dn, cn = dets.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(cn, o["counts"]) and np.array_equal(cn, h["counts"])
    tol = 1e-4 * max(RC.FRAME)          # float32 boxes of up to 200 px through an exp and a few products: well under 1e-4 relative
    for b in range(c.B):
        n = int(cn[b, 0])
        assert dn[b, :n, 5].astype(int).tolist() == o["classes"][b] == h["dets"][b, :n, 5].astype(int).tolist()
        for want in (o["dets"], h["dets"]):                               # the kept order: row by row the oracle's and the host's
            assert np.abs(dn[b, :, :5] - want[b, :, :5]).max() <= tol
        assert (dn[b, n:] == 0).all()


@pytest.mark.parametrize("name", [n for n, *_ in RC.post_exact_inputs()])
def test_output_stage_exact_decisions_by_hand(RO, host, name):
    """p exactly at conf_thr is dropped (>) and kept one float32 step below; of classes with the same probability the lowest
    wins: the rows written out by hand in rcnn_cases.post_exact_inputs, and the host build's bits."""
    _, c, inputs, dets, counts = next(q for q in RC.post_exact_inputs() if q[0] == name)
    got_d, got_c = _post_raw(RO, c, inputs=inputs)
    h = RC.host_post(host, c, inputs=inputs)
    assert np.array_equal(got_c.cpu().numpy(), counts) and np.array_equal(h["counts"], counts)
    assert _bits(got_d) == dets.tobytes() == h["dets"].tobytes()


def test_output_stage_drops_non_finite_logits(RO, host):
    """A row of NaN logits and a row with a +inf logit in image 0 are dropped; image 1's rows and counts keep their bits."""
    c, clean, bad = RC.post_poison_inputs()
    o = RC.oracle_post(*bad, c.conf, RC.IOU_THR, c.max_det)
    hb = RC.host_post(host, c, inputs=bad)
    (d0, c0), (d1, c1) = _post_raw(RO, c, inputs=clean), _post_raw(RO, c, inputs=bad)
    assert _bits(d0[1]) == _bits(d1[1]) and _bits(c0[1]) == _bits(c1[1]) and torch.isfinite(d1).all()
    cn, dn = c1.cpu().numpy(), d1.cpu().numpy()
    assert np.array_equal(cn, o["counts"]) and np.array_equal(cn, hb["counts"]) and cn[0, 1] == int(c0[0, 1]) - 2
    n = int(cn[0, 0])
    assert dn[0, :n, 5].astype(int).tolist() == o["classes"][0] == hb["dets"][0, :n, 5].astype(int).tolist()
    for want in (o["dets"], hb["dets"]):
        assert np.abs(dn[0, :, :5] - want[0, :, :5]).max() <= 1e-4 * max(RC.FRAME)
    assert (dn[0, n:] == 0).all()


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

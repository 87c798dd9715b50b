"""The two-stage detector stage without a device: the oracle of tests/rcnn_cases.py keeps its own margins and is checked
against independent formulations (the sampler's ranks against sorted() on the keys, RoIAlign against F.grid_sample with
border padding plus the outside-range mask, its gradient by the transpose identity), and the host build of csrc/gsr_rcnn.h
(tests/host_math/rcnn_host.cpp) -- the scalar source the kernels compile -- matches the oracle: integers equal, floats
within detloss_cases.bound of the float32 yardstick."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rcnn_cases as RC


@pytest.fixture(scope="module")
def host():
    return RC.host_lib()


def _report(who, cid, got, ref, keys):
    fails = []
    for k in keys:
        e, y = RC.err(got[k], ref["o64"][k]), ref["yard"][k]
        b = RC.bound(y)
        print(f"{who} {cid} {k}: err {e:.3e} yardstick {y:.3e} bound {b:.3e}")
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, f"{who} {cid}: {fails}"


# ---- the sampler --------------------------------------------------------------------------------------------------------------
def test_mix32_literals():
    assert RC.mix32(0) == 0 and RC.mix32(1) == 0x688990c0 and RC.sample_key(7, 1, 5) == 0xb0dcbc63
    seen = {RC.sample_key(7, b, i) for b in range(2) for i in range(4096)}
    assert len(seen) > 8180                                              # a 32-bit mix: (almost) no two candidates share a key
    assert RC.sample_key(7, 0, 5) != RC.sample_key(8, 0, 5) and RC.sample_key(7, 0, 5) != RC.sample_key(7, 1, 5)


@pytest.mark.parametrize("c", RC.SAMPLE_CASES, ids=lambda c: c.id)
def test_sampler_oracle_keeps_its_margins_and_contract(c):
    o = RC.sample_reference(c)
    print(f"{c.id}: gap_fg {o['gap_fg']:.3e} gap_lead {o['gap_lead']:.3e} counts {o['counts'].tolist()}")
    assert RC.sample_margins_ok(o)
    N = c.R + (c.M if c.append_gt else 0)
    for b in range(RC.B):
        n, npos = (int(v) for v in o["counts"][b])
        idx = o["idx"][b]
        assert (np.diff(idx[:n]) > 0).all() and (idx[n:] == -1).all() and (0 <= idx[:n]).all() and (idx[:n] < N).all()
        assert (o["labels"][b, n:] == -1).all() and (o["gt_row"][b, n:] == -1).all() and (o["rois"][b, n:] == 0).all()
        assert int((o["labels"][b, :n] < RC.NC).sum()) == npos == int((o["gt_row"][b, :n] >= 0).sum())
        # the ranks, in plain Python: the taken of a kind are the first of sorted() on (key, index)
        for kind, quota in ((True, npos), (False, n - npos)):
            members = [i for i in range(N) if o["kinds"][b][i] is kind]
            first = sorted(members, key=lambda i: (o["keys"][b][i], i))[:quota]
            took = [int(i) for i in idx[:n] if o["kinds"][b][int(i)] is kind]
            assert sorted(first) == took


def test_sampler_cases_cover_what_they_claim():
    ref = {c.id: RC.sample_reference(c) for c in RC.SAMPLE_CASES}
    c0 = ref["both-quotas"]
    kinds = c0["kinds"][0]
    assert sum(k is True for k in kinds) > 1 and sum(k is False for k in kinds) > 3         # both quotas bite (image 0)
    assert (c0["counts"] == np.array([[4, 1], [4, 1]])).all()
    assert (ref["all-taken"]["counts"][:, 0] == 8).all() and (ref["all-taken"]["idx"][:, 8:] == -1).all()
    assert ref["n4096"]["counts"][:, 0].tolist() == [1024, 1024] and ref["n1025"]["counts"][:, 0].tolist() == [512, 512]
    assert ref["n-prop"]["idx"][0].max() >= 70 and (ref["n-prop"]["idx"][0][ref["n-prop"]["idx"][0] < 70] < 40).all()
    assert ref["n-prop"]["counts"][1].tolist() == [3, 3]                 # image 1: the ground-truth rows alone
    assert ref["absent-rows"]["counts"][1, 1] == 0 and (ref["absent-rows"]["labels"][1, :32] == RC.NC).all()
    assert (ref["absent-rows"]["gt_row"][0] <= 0).all()
    assert ref["no-append"]["idx"].max() < 70
    assert ref["gt-only-fg"]["counts"][:, 1].tolist() == [1, 1] and ref["gt-only-fg-no-append"]["counts"][:, 1].tolist() == [0, 0]
    c = RC.SAMPLE_CASES[2]
    a, b_, a2 = RC.sample_reference(c, 1), RC.sample_reference(c, 2), RC.oracle_sample(*RC.sample_inputs(c), RC.NC, c.S, c.max_pos, True, 1)
    assert not np.array_equal(a["idx"], b_["idx"]) and np.array_equal(a["idx"], a2["idx"])
    # candidates per lane of the kernel's 1024: per = ceil(N / 1024), reached at its first and its full N
    per = {c.id: -(-(c.R + c.M) // 1024) for c in RC.SAMPLE_CASES}
    assert [per[k] for k in ("n1024", "n1025", "n2049", "n3072", "n3073", "n4096")] == [1, 2, 3, 3, 4, 4]
    assert RC.SAMPLE_CASES[10].R + RC.SAMPLE_CASES[10].M == 1024 and RC.SAMPLE_CASES[10].id == "n1024"
    for k in ("n1024", "n2049", "n3072", "n3073"):                       # both quotas bite in both images
        for b in range(RC.B):
            kinds = ref[k]["kinds"][b]
            assert sum(q is True for q in kinds) > 128 and sum(q is False for q in kinds) > 384, k
        assert ref[k]["counts"].tolist() == [[512, 128]] * 2, k


def test_sampler_exact_decisions_by_hand(host):
    """An IoU of exactly fg_iou is foreground, of two identical present rows the lower one is the match, an absent row in front
    of them is skipped: the oracle in both precisions and the host build give the rows written out by hand."""
    c, inputs, want = RC.sample_exact_inputs()
    prop, gt, cls, n_prop = inputs
    for dtype in (torch.float64, torch.float32):
        iou = RC.pair_iou(torch.tensor(prop[0]).to(dtype), torch.tensor(gt[0]).to(dtype))
        assert float(iou[0, 1]) == 0.5 and float(iou[1, 1]) == 1.0 and abs(float(iou[2, 1]) - 0.4) < 1e-6 and float(iou[3, 1]) == 0.0
        o = RC.oracle_sample(prop, gt, cls, n_prop, RC.NC, c.S, c.max_pos, c.append_gt, c.seed, dtype=dtype)
        for k, w in want.items():
            assert np.array_equal(o[k], w), (dtype, k)
    h = RC.host_sample(host, c, inputs=inputs)
    for k, w in want.items():
        assert np.array_equal(h[k], w), k
    assert h["rois"].tobytes() == o["rois"].tobytes()


def test_sampler_keys_of_one_image_never_tie():
    """key_before's index tie-break cannot decide anything within one image: mix32 is a bijection of the 32-bit words (two
    xor-shifts and two odd multipliers, each invertible), so sample_key(seed, b, .) maps distinct indices to distinct keys.
    Checked here for a few seeds over all 4096 indices; a search of the seeds below 10 000 found no pair either."""
    for seed in (0, 7, 11, 9999):
        for b in range(2):
            assert len({RC.sample_key(seed, b, i) for i in range(4096)}) == 4096


@pytest.mark.parametrize("c", RC.SAMPLE_CASES, ids=lambda c: c.id)
def test_host_sampler_equals_the_oracle(host, c):
    o, h = RC.sample_reference(c), RC.host_sample(host, c)
    for k in ("idx", "labels", "gt_row", "counts"):
        assert np.array_equal(h[k], o[k]), f"{c.id}: {k} differs"
    assert h["rois"].tobytes() == o["rois"].tobytes()


# ---- RoIAlign -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.ROI_CASES, ids=lambda c: c.id)
def test_roi_oracle_margins_and_host_build(host, c):
    ref = RC.roi_reference(c)
    print(f"{c.id}: gap_grid {ref['gap_grid']:.3e} grids {ref['o64']['grids'][0].tolist()}")
    assert RC.roi_margins_ok(ref)
    h = RC.host_roi(host, c)
    _report("host", c.id, h, ref, ("pooled", "grad_features"))
    p = ref["o64"]["pooled"]
    assert all(bool((p[b, s] == 0).all()) for b, s in RC.roi_dead_rows(c))
    assert all((h["pooled"][b, s] == 0).all() for b, s in RC.roi_dead_rows(c))
    if c.table != "base":
        return
    _report("host scatter", c.id, dict(grad_features=h["scatter"]), ref, ("grad_features",))    # the other order of the same sum
    assert (p[0, 7] == 0).all() and (p[1, 7:] == 0).all()                 # the NaN row and the rows beyond n_roi
    g = ref["o64"]["grids"][0]
    if c.ratio == 0:
        assert tuple(g[3]) == (0, 0) and (p[0, 3] == 0).all()             # zero area
        assert g[6][1] == 16 and g[5].min() >= (1 if c.PH == 14 else 2)   # the cap; the whole map
    assert float(p[0, 1].abs().max()) > 0 and float(p[0, 2].abs().max()) > 0


def test_roi_oracle_against_grid_sample():
    """An independent formulation of the bilinear read: for samples in [-1, Hf] border padding reproduces the clamp at 0 and
    the y_low >= Hf - 1 branch; outside, the read is 0."""
    c = RC.RoiCase(3, 3, 5, 2)
    feat, _ = RC.roi_inputs(c.Cf, c.PH, c.PW)
    f = torch.tensor(feat).double()
    pooled, _, _ = RC.oracle_roi_align(f, RC.ROIS, RC.N_ROI, 2, c.PH, c.PW, RC.SCALE, c.ratio)
    sc = float(np.float32(RC.SCALE))
    for b, s in ((0, 0), (0, 1), (0, 2), (0, 4), (0, 5), (1, 0), (1, 3)):
        r = torch.tensor(RC.ROIS[b, s]).double()
        sx, sy = r[0] * sc - 0.5, r[1] * sc - 0.5
        bx, by = (r[2] * sc - 0.5 - sx) / c.PW, (r[3] * sc - 0.5 - sy) / c.PH
        g = c.ratio
        ys = (sy + torch.arange(c.PH).double()[:, None] * by + (torch.arange(g).double()[None, :] + 0.5) * by / g).reshape(-1)
        xs = (sx + torch.arange(c.PW).double()[:, None] * bx + (torch.arange(g).double()[None, :] + 0.5) * bx / g).reshape(-1)
        gy, gx = torch.meshgrid(ys, xs, indexing="ij")
        grid = torch.stack([2 * gx / (RC.WF - 1) - 1, 2 * gy / (RC.HF - 1) - 1], -1)[None]
        v = F.grid_sample(f[b:b + 1], grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        ok = (gy >= -1) & (gy <= RC.HF) & (gx >= -1) & (gx <= RC.WF)
        v = torch.where(ok[None], v, torch.zeros_like(v))
        want = v.reshape(c.Cf, c.PH, g, c.PW, g).sum(dim=(2, 4)) / (g * g)
        assert torch.allclose(pooled[b, s], want, rtol=1e-12, atol=1e-12), (b, s)


def test_roi_oracle_gradient_is_the_transpose():
    c = RC.RoiCase(3, 7, 7, 0)
    o = RC.roi_reference(c)["o64"]
    feat, gp = RC.roi_inputs(c.Cf, c.PH, c.PW)
    lhs = (o["pooled"] * torch.tensor(gp).double()).sum()
    rhs = (o["grad_features"] * torch.tensor(feat).double()).sum()         # the map is linear in the features
    assert abs(float(lhs - rhs)) <= 1e-10 * abs(float(lhs))


def test_roi_cases_cover_what_they_claim():
    by = {c.id: c for c in RC.ROI_CASES}
    # the wide map: 2 x 4 tiles, and per RoI most of them skipped -- by the span test restated in float32 and in float64
    w = by["wide-c3-r2"]
    tiles = [(y0, x0) for y0 in range(0, w.Hf, 8) for x0 in range(0, w.Wf, 8)]
    assert len(tiles) == 8 and len({x for _, x in tiles}) == 4 and len({y for y, _ in tiles}) == 2
    rois, n_roi = RC.roi_table(w)
    assert n_roi[:, 0].tolist() == [13, 5]
    walked = {}
    for b in range(2):
        for s in range(int(n_roi[b, 0])):
            walked[b, s] = RC.tiles_walked(w, rois[b, s])
            assert walked[b, s] == RC.tiles_walked(w, rois[b, s], np.float64), (b, s)
    skipped = [8 - len(v) for v in walked.values()]
    print("wide: tiles skipped per RoI", skipped)
    assert sum(k >= 4 for k in skipped) > len(skipped) // 2                  # most RoIs are skipped by most tiles
    assert all((0, 24) not in walked[0, s] for s in (0, 1, 5, 7)) and (0, 24) in walked[0, 3] and (8, 24) in walked[0, 12]
    assert (0, 0) not in walked[0, 2] and (0, 0) not in walked[0, 3]
    # the rows on the span test's edges: equal spans but for the edge, on either side of it
    x = lambda s, dt: RC.roi_span(rois[0, s], w.scale, w.PH, w.PW, dt)[2:]
    for dt in (np.float32, np.float64):
        assert x(5, dt) == (7.0, 1.0) and x(6, dt) == (9.0, 1.0)               # spans [7, 14] and [9, 16], exactly
        assert not RC.span_misses(*x(5, dt), 7, 16, dt) and RC.span_misses(*x(7, dt), 7, 16, dt)    # hi == c0 - 2: walked; below: skipped
        assert not RC.span_misses(*x(6, dt), 7, 0, dt) and RC.span_misses(*x(8, dt), 7, 0, dt)      # lo == c0 + 9: walked; above: skipped
    assert (0, 16) in walked[0, 5] and (0, 16) not in walked[0, 7] and (0, 0) in walked[0, 6] and (0, 0) not in walked[0, 8]
    # inverted rows: samples that run backwards at a fixed ratio, a grid of 0 when adaptive
    fixed, adaptive = RC.roi_reference(w)["o64"], RC.roi_reference(by["wide-c1-r0"])["o64"]
    for b, s in RC.WIDE_INVERTED:
        r = rois[b, s]
        assert r[2] < r[0] or r[3] < r[1]
        assert float(fixed["pooled"][b, s].abs().max()) > 0 and (fixed["grids"][b, s] == 2).all()
        assert (adaptive["pooled"][b, s] == 0).all() and adaptive["grids"][b, s].min() == 0
    assert rois[0, 9, 2] < rois[0, 9, 0] and rois[0, 9, 3] > rois[0, 9, 1] and rois[0, 10, 3] < rois[0, 10, 1] and (rois[0, 11, 2:] < rois[0, 11, :2]).all()
    # the fixed ratio reaches MAX_GRID itself; Cf at the edges of the backward's 32-channel chunk
    assert (RC.roi_reference(by["wide-c33-r16"])["o64"]["grids"][0, :9] == 16).all()
    assert {by[f"wide-c{cf}-r1"].Cf for cf in (1, 32, 33)} == {1, 32, 33}
    # an image with count 0: its gradient is zero, the other image's is not
    z = by["wide-zero-c33-r0"]
    assert RC.roi_table(z)[1][:, 0].tolist() == [13, 0]
    gz = RC.roi_reference(z)["o64"]["grad_features"]
    assert (gz[1] == 0).all() and float(gz[0].abs().max()) > 0
    # maps with a side of 1, sides that are multiples of the tile, other scales, flat bins, S = 1024
    assert [(by[k].Hf, by[k].Wf) for k in ("h1-r0", "w1-r0", "one-r0", "mult8-r0")] == [(1, 11), (9, 1), (1, 1), (8, 16)]
    assert (by["scale-1"].scale, by["scale-quarter"].scale) == (1.0, 0.25) and (by["scale-1"].Hf, by["scale-1"].Wf) == (16, 24)
    assert (by["14x1-r0"].PH, by["14x1-r0"].PW, by["1x14-r2"].PH, by["1x14-r2"].PW) == (14, 1, 1, 14)
    for k in ("h1-r0", "w1-r2", "one-r0", "one-r2", "mult8-r0", "scale-1", "scale-quarter", "14x1-r0", "1x14-r2"):
        o = RC.roi_reference(by[k])["o64"]
        live = [(b, s) for b in range(2) for s in range(by[k].S) if (b, s) not in RC.roi_dead_rows(by[k])]
        assert sum(float(o["pooled"][b, s].abs().max()) > 0 for b, s in live) >= len(live) // 2, k
        assert float(o["grad_features"].abs().max()) > 0
    big = by["s1024"]
    rois, n_roi = RC.roi_table(big)
    assert rois.shape == (2, 1024, 4) and n_roi[:, 0].tolist() == [1000, 0]
    o = RC.roi_reference(big)["o64"]
    assert float(o["pooled"][0, 999].abs().max()) > 0 and (o["pooled"][0, 1000:] == 0).all() and (o["pooled"][1] == 0).all()


def test_roi_exact_edges_by_hand(host):
    """A sample at exactly -1 or exactly n is valid and reads the border cell with weight 1; the next representable position
    further out reads 0.  The positions are the same in float32 and float64, the oracle in both precisions and the host build
    give the values written out by hand, and the backward is the transposed statement."""
    c, inputs, pooled, gf, cells = RC.roi_edge_inputs()
    feat, gp, rois, n_roi = inputs
    for s, cell in enumerate(cells):
        x1, y1, x2, y2 = (float(v) for v in rois[0, s])
        for dt in (np.float32, np.float64):
            py, px = float(RC.edge_pos(y1, y2, dt)), float(RC.edge_pos(x1, x2, dt))
            if cell is not None:
                assert (py, px) == (-1.0 if cell[0] == 0 else c.Hf, -1.0 if cell[1] == 0 else c.Wf), (s, dt)
            else:
                assert py < -1.0 or py > c.Hf or px < -1.0 or px > c.Wf, (s, dt)
                assert abs(py - round(py)) < 1e-6 and abs(px - round(px)) < 1e-6      # a step or two outside, no more
    for dtype in (torch.float64, torch.float32):
        f = torch.tensor(feat).to(dtype).requires_grad_(True)
        p, _, _ = RC.oracle_roi_align(f, rois, n_roi, 2, 1, 1, c.scale, c.ratio, dtype)
        (p * torch.tensor(gp).to(dtype)).sum().backward()
        assert np.array_equal(p.detach().numpy()[0, :, :, 0, 0], pooled) and np.array_equal(f.grad.numpy()[0], gf), dtype
    h = RC.host_roi(host, c, inputs=inputs)
    assert np.array_equal(h["pooled"][0, :, :, 0, 0], pooled) and np.array_equal(h["grad_features"][0], gf)
    assert np.array_equal(h["scatter"][0], gf)


# ---- the loss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.LOSS_CASES, ids=lambda c: c.id)
def test_host_loss_matches_the_oracle(host, c):
    ref, i = RC.loss_reference(c), RC.loss_inputs(c)
    _report("host", c.id, RC.host_loss(host, c), ref, RC.LOSS_COMPARED)
    h64 = RC.host_loss(host, c, double=True)
    for k in RC.LOSS_COMPARED:
        assert RC.err(h64[k], ref["o64"][k]) <= 1e-12, k
    assert RC.host_loss(host, c, want_grad=False)["loss"].tobytes() == RC.host_loss(host, c)["loss"].tobytes()
    o = ref["o64"]
    labels = i["labels"]
    assert (o["grad_scores"][torch.tensor(labels < 0)] == 0).all()
    if c.all_bg:
        assert float(o["loss"][1]) == 0 and (o["grad_deltas"] == 0).all() and (labels[labels >= 0] == c.C).all()
    elif not c.pad_image:
        assert float(o["loss"][1]) > 0 and i["zero_row"] is not None
        b, s = i["zero_row"]
        assert (o["grad_deltas"][b, s] == 0).all()                        # a residual of exactly 0: sign(0) = 0
    if c.pad_image:
        assert (labels[1] == -1).all() and (labels[0] >= 0).all()


def test_loss_cases_cover_what_they_claim():
    by = {c.id: c for c in RC.LOSS_CASES}
    rows = {k: c.B * c.S for k, c in by.items()}
    assert rows["rows-33"] == 33 and rows["rows-33"] % 4 == 1                 # the last block of four waves holds one row
    assert (rows["s1024"] + 3) // 4 == 512 > 256 and rows["s1024"] // 256 == 8  # slab_sum turns twice, k_rcnn_count eight times
    assert int((RC.loss_inputs(by["s1024"])["labels"] >= 0).sum()) == 2048 and int((RC.loss_inputs(by["s1024"])["gt_row"] >= 0).sum()) > 256
    assert [by[k].C + 1 for k in ("c63", "c64", "c65", "c1024")] == [64, 65, 66, 1025]      # logits per row, around a wave's 64
    assert by["c1024-agnostic"].agnostic and by["c1024-agnostic"].C == 1024
    for k in ("c63", "c64", "c65", "c1024", "c1024-agnostic"):
        c, i = by[k], RC.loss_inputs(by[k])
        seen = set(i["labels"].reshape(-1).tolist())
        assert {0, c.C - 1, c.C} <= seen and len(seen) >= 6, (k, sorted(seen))  # the whole class range, its last class, background
        assert max(v for v in seen if v < c.C - 1) > c.C // 2


def test_host_loss_guards(host):
    """A label above C counts as -1 (the same bits as -1 itself, with 2^31 - 1 and -7 beside it); a foreground row whose gt_row
    is M, M + 100 or -3 keeps its cross-entropy term and gradient, adds nothing to the box term and has a zero grad_deltas row."""
    c, base, bad_lb, clean_lb, bad_gr, rows = RC.loss_guard_inputs()
    a, b_ = RC.host_loss(host, c, inputs=bad_lb), RC.host_loss(host, c, inputs=clean_lb)
    for k in RC.LOSS_COMPARED:
        assert a[k].tobytes() == b_[k].tobytes() and np.isfinite(a[k]).all(), k
    _report("host", "clean-labels", b_, RC.loss_reference_of(c, clean_lb), RC.LOSS_COMPARED)
    assert b_["loss"].tobytes() != RC.host_loss(host, c)["loss"].tobytes()
    ref, g, h0 = RC.loss_reference_of(c, bad_gr), RC.host_loss(host, c, inputs=bad_gr), RC.host_loss(host, c)
    _report("host", "bad-rows", g, ref, RC.LOSS_COMPARED)
    assert g["loss"][0] == h0["loss"][0] and g["loss"][1] < h0["loss"][1] and g["grad_scores"].tobytes() == h0["grad_scores"].tobytes()
    for k in RC.LOSS_COMPARED:
        assert np.isfinite(g[k]).all() and bool(torch.isfinite(ref["o64"][k]).all())
    for b, s in rows:
        assert (g["grad_deltas"][b, s] == 0).all() and (ref["o64"]["grad_deltas"][b, s] == 0).all()
        assert np.abs(h0["grad_deltas"][b, s]).max() > 0 and np.abs(g["grad_scores"][b, s]).max() > 0
    h64 = RC.host_loss(host, c, double=True, inputs=bad_gr)
    for k in RC.LOSS_COMPARED:
        assert RC.err(h64[k], ref["o64"][k]) <= 1e-12, k


# ---- the output stage ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RC.POST_CASES, ids=lambda c: c.id)
def test_host_output_stage_equals_the_oracle(host, c):
    o, h = RC.post_reference(c), RC.host_post(host, c)
    print(f"{c.id}: gap_conf {o['gap_conf']:.3e} gap_nms {o['gap_nms']:.3e} counts {o['counts'].tolist()} order {o['order']}")
    assert RC.post_margins_ok(o)
    assert np.array_equal(h["counts"], o["counts"])
    for b in range(RC.B):
        n = int(o["counts"][b, 0])
        assert h["dets"][b, :n, 5].astype(int).tolist() == o["classes"][b]
        assert np.abs(h["dets"][b, :, :5] - o["dets"][b, :, :5]).max() <= 1e-4 * max(RC.FRAME)
        assert (h["dets"][b, n:] == 0).all()


def test_output_cases_cover_what_they_claim():
    lo, hi, many = (RC.post_reference(c) for c in (RC.POST_CASES[0], RC.POST_CASES[1], RC.POST_CASES[3]))
    assert lo["order"][0][:4] == [9, 4, 0, 1]                             # two classes on one box (0, 1): both kept
    assert 2 in lo["order"][0] and 3 not in lo["order"][0]                # one class overlapping: one kept
    assert 10 not in lo["order"][0] and 11 not in lo["order"][0] and 11 in lo["order"][1]     # non-finite; beyond n_prop
    assert lo["counts"][0, 1] > hi["counts"][0, 1] and 5 in lo["order"][0] and 5 not in hi["order"][0]
    d = lo["dets"][0]
    assert tuple(d[1, :4]) == (0.0, 0.0, RC.FRAME[0], RC.FRAME[1])        # the dw clamp reached, clipped on all four sides
    assert many["counts"].tolist() == [[5, 40], [0, 0]]                   # more than max_det candidates; no candidate
    by = {c.id: c for c in RC.POST_CASES}
    per = {k: -(-by[k].R // 1024) for k in ("r1024", "r1025", "r2049", "r4096")}
    assert per == {"r1024": 1, "r1025": 2, "r2049": 3, "r4096": 4}
    for k, p in per.items():
        c, o, cand = by[k], RC.post_reference(by[k]), RC.post_candidates(by[k])
        n_prop = RC.post_inputs(c)[3]
        assert n_prop[0] == c.R and 0 < n_prop[1] < c.R
        for b in range(2):
            assert len(cand[b]) == c.ncand == int(o["counts"][b, 1]) and c.ncand >= 200
            assert {i for i in (0, 1023, 1024, c.R - 1) if i < n_prop[b]} <= set(cand[b])
            assert min(cand[b]) == 0 and max(cand[b]) >= n_prop[b] - 40 and len({i * 8 // c.R for i in cand[b]}) == 8     # the whole range
            assert {i % p for i in cand[b]} == set(range(p))                 # a candidate in every slot k of i = t * per + k
            kept, order = int(o["counts"][b, 0]), o["order"][b]
            assert kept == len(order) < c.ncand or kept == c.max_det
        # the NMS walk suppresses within at least two classes: candidates that score above the last kept one and are not kept
        scores = torch.softmax(torch.tensor(np.array(RC.post_inputs(c)[0])).double(), -1)[..., :c.C]
        for b in range(2):
            best, last = scores[b].max(-1).values, min(float(scores[b, i].max()) for i in o["order"][b])
            lost = [int(scores[b, i].argmax()) for i in cand[b] if i not in o["order"][b] and float(best[i]) > last]
            assert len(set(lost)) >= 2 and len(lost) >= 10, (k, b, lost)
    full = RC.post_candidates(by["r4096"])
    assert any(all(4 * t + q in set(full[b]) for q in range(4)) for b in range(2) for t in range(1024))       # all four slots of one thread
    assert -(-by["r1025"].R // 2) == 513                                  # per = 2: the threads from 513 on hold no proposal
    assert by["r4096"].max_det > 256 and int(RC.post_reference(by["r4096"])["counts"][:, 0].max()) > 256       # k_rcnn_gather's second trip
    for k in ("c64", "c1024"):
        o, c = RC.post_reference(by[k]), by[k]
        seen = {q for b in range(2) for q in o["classes"][b]}
        assert {0, c.C - 1} <= seen and len(seen) > 5, (k, sorted(seen))
    assert by["maxdet-1"].max_det == 1 and RC.post_reference(by["maxdet-1"])["counts"][:, 0].tolist() == [1, 1]
    r40 = RC.post_reference(by["maxdet-R"])
    assert by["maxdet-R"].max_det == 40 == RC.post_inputs(by["maxdet-R"])[0].shape[1] and r40["counts"][0].tolist() == [40, 40]
    e = by["b3-empty-middle"]
    assert RC.post_inputs(e)[3][1] == 0 and RC.post_reference(e)["counts"][:, 1].tolist() == [30, 0, 30]
    assert len(RC.post_candidates(PostEmptyProbe(e))[1]) == 30            # ... whose rows would be candidates if they counted


def PostEmptyProbe(c):
    """The case with no image empty: the same rows (the generator draws an empty image's rows as if it were full)."""
    return c._replace(empty=())


@pytest.mark.parametrize("name", [n for n, *_ in RC.post_exact_inputs()])
def test_host_output_exact_decisions_by_hand(host, name):
    """p exactly at conf_thr is dropped and kept one float32 step below; of classes with the same probability the lowest wins;
    the oracle in both precisions and the host build give the rows written out by hand."""
    _, c, inputs, dets, counts = next(q for q in RC.post_exact_inputs() if q[0] == name)
    for dtype in (torch.float64, torch.float32):
        o = RC.oracle_post(*inputs, c.conf, RC.IOU_THR, c.max_det, dtype=dtype)
        assert np.array_equal(o["counts"], counts) and np.array_equal(o["dets"], dets.astype(np.float64)), dtype
    h = RC.host_post(host, c, inputs=inputs)
    assert np.array_equal(h["counts"], counts) and h["dets"].tobytes() == dets.tobytes()


def test_host_output_drops_non_finite_logits(host):
    c, clean, bad = RC.post_poison_inputs()
    o, ob = RC.post_reference(c), RC.oracle_post(*bad, c.conf, RC.IOU_THR, c.max_det)
    h, hb = RC.host_post(host, c), RC.host_post(host, c, inputs=bad)
    assert 8 in o["order"][0] and 9 in o["order"][0] and 8 not in ob["order"][0] and 9 not in ob["order"][0]
    assert ob["counts"][0, 1] == o["counts"][0, 1] - 2 and np.array_equal(hb["counts"], ob["counts"])
    assert hb["dets"][1].tobytes() == h["dets"][1].tobytes() and np.isfinite(hb["dets"]).all()
    n = int(ob["counts"][0, 0])
    assert hb["dets"][0, :n, 5].astype(int).tolist() == ob["classes"][0] and (hb["dets"][0, n:] == 0).all()
    assert np.abs(hb["dets"][0, :, :5] - ob["dets"][0, :, :5]).max() <= 1e-4 * max(RC.FRAME)

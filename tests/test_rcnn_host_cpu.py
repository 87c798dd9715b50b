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
    _report("host", c.id, RC.host_roi(host, c), ref, ("pooled", "grad_features"))
    p = ref["o64"]["pooled"]
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

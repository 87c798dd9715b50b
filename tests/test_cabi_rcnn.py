"""The two-stage detector stage's C ABI and Python surface, the parts that need no GPU: symbols, the capability bit next to
the unchanged bits and version, the struct layout, every argument check (refused before any device call: the pointers
handed over are never followed), the workspace size, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import rcnn_ops as RO
from gsplat_attack import roi_detector as RD

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return RO._lib()


def _spec(**kw):
    cs = RO.c_spec(RO.RcnnSpec(S=16, max_pos=4, max_det=8, img_w=640.0, img_h=480.0), B=2, R=32, M=2, C=3, Cf=8, Hf=9, Wf=11)
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


def _ref(cs):
    return ctypes.byref(cs) if cs is not None else None


def _sample(lib, cs, prop=FAKE, n_prop=None, gtb=FAKE, gtc=FAKE, idx=FAKE, rois=FAKE, labels=FAKE, gt_row=FAKE, counts=FAKE):
    return lib.gsr_rcnn_sample(_ref(cs), prop, n_prop, gtb, gtc, idx, rois, labels, gt_row, counts, None)


def _fwd(lib, cs, feat=FAKE, rois=FAKE, n_roi=None, stride=0, pooled=FAKE):
    return lib.gsr_roi_align(_ref(cs), feat, rois, n_roi, stride, pooled, None)


def _bwd(lib, cs, rois=FAKE, n_roi=None, stride=0, gp=FAKE, gf=FAKE):
    return lib.gsr_roi_align_backward(_ref(cs), rois, n_roi, stride, gp, gf, 0, None)


def _loss(lib, cs, scores=FAKE, deltas=FAKE, rois=FAKE, labels=FAKE, gt_row=FAKE, gtb=FAKE, ws=FAKE, ws_bytes=BIG, loss=FAKE, gs=FAKE,
          gd=FAKE):
    return lib.gsr_rcnn_loss(_ref(cs), scores, deltas, rois, labels, gt_row, gtb, ws, ws_bytes, loss, gs, gd, None)


def _post(lib, cs, scores=FAKE, deltas=FAKE, prop=FAKE, n_prop=None, ws=FAKE, ws_bytes=BIG, dets=FAKE, counts=FAKE):
    return lib.gsr_rcnn_postprocess(_ref(cs), scores, deltas, prop, n_prop, ws, ws_bytes, dets, counts, None)


CALLS = {"gsr_rcnn_sample": _sample, "gsr_roi_align": _fwd, "gsr_roi_align_backward": _bwd, "gsr_rcnn_loss": _loss,
         "gsr_rcnn_postprocess": _post}


def test_symbols_version_and_capability(lib):
    for name, n in (("gsr_rcnn_sample", 11), ("gsr_roi_align", 7), ("gsr_roi_align_backward", 8), ("gsr_rcnn_workspace_bytes", 2),
                    ("gsr_rcnn_loss", 13), ("gsr_rcnn_postprocess", 10)):
        assert len(getattr(lib, name).argtypes) == n
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(3, ctypes.byref(out)) == 0 and out.value == 15          # closed at bits 0..3: compared as a whole elsewhere
    assert lib.gsr_query(4, ctypes.byref(out)) == 0 and out.value == 15 | 16     # every capability bit
    assert RO.available() and RO.GSR_CAP_RCNN == 16
    names = [f[0] for f in RO._CRcnnSpec._fields_]
    assert names[:9] == ["B", "R", "M", "S", "C", "max_pos", "append_gt", "seed", "fg_iou"] and names[-1] == "flags"
    assert ctypes.sizeof(RO._CRcnnSpec) == 4 * len(names) == 116
    assert [getattr(RO._CRcnnSpec, n).offset for n in names] == list(range(0, 116, 4))
    d = RO.RcnnSpec()
    assert (d.S, d.max_pos, d.fg_iou, d.PH, d.PW, d.spatial_scale, d.sampling_ratio) == (512, 128, 0.5, 14, 14, 1 / 16, 0)
    assert (d.box_weights, d.beta, d.w_cls, d.w_box, d.conf_thr, d.iou_thr, d.max_det) == ((10, 10, 5, 5), 0, 1, 0, 0.5, 0.5, 100)


BAD = {
    "gsr_rcnn_sample": [dict(B=0), dict(B=65536), dict(flags=2), dict(M=0), dict(M=33), dict(S=0), dict(S=1025), dict(C=0), dict(C=1025),
                        dict(R=0), dict(R=4095), dict(max_pos=-1), dict(max_pos=17), dict(fg_iou=NAN), dict(fg_iou=-0.1)],
    "gsr_roi_align": [dict(B=0), dict(flags=0x80000000), dict(S=0), dict(S=1025), dict(Cf=0), dict(Hf=0), dict(Wf=-1), dict(PH=0), dict(PH=15),
                      dict(PW=0), dict(PW=15), dict(sampling_ratio=-1), dict(spatial_scale=0.0), dict(spatial_scale=NAN),
                      dict(spatial_scale=INF), dict(B=64, S=1024, Cf=1024, PH=14, PW=14)],
    "gsr_rcnn_loss": [dict(B=0), dict(flags=4), dict(S=0), dict(S=1025), dict(M=0), dict(M=33), dict(C=0), dict(C=1025), dict(bw_x=0.0),
                      dict(bw_y=-1.0), dict(bw_w=NAN), dict(bw_h=INF), dict(beta=-0.5), dict(beta=NAN), dict(w_cls=-1.0), dict(w_box=INF)],
    "gsr_rcnn_postprocess": [dict(B=0), dict(flags=2), dict(R=0), dict(R=4097), dict(C=0), dict(max_det=0), dict(max_det=33), dict(bw_w=0.0),
                             dict(conf_thr=NAN), dict(conf_thr=-0.1), dict(iou_thr=INF), dict(img_w=0.0), dict(img_h=NAN), dict(img_h=-4.0)],
}
BAD["gsr_roi_align_backward"] = BAD["gsr_roi_align"]


@pytest.mark.parametrize("fn", sorted(BAD))
def test_spec_checks(lib, fn):
    for bad in BAD[fn]:                                    # (a valid spec is never sent with the fake pointers)
        assert CALLS[fn](lib, _spec(**bad)) == INVALID, (fn, bad)
        assert fn.encode() + b":" in lib.gsr_last_error(), (fn, bad)
    assert CALLS[fn](lib, None) == INVALID and b"null spec" in lib.gsr_last_error()


def test_null_and_misaligned_pointers_and_workspaces(lib):
    cs = _spec()
    for fn, names in (("gsr_rcnn_sample", ("prop", "gtb", "gtc", "idx", "rois", "labels", "gt_row", "counts")),
                      ("gsr_roi_align", ("feat", "rois", "pooled")), ("gsr_roi_align_backward", ("rois", "gp", "gf")),
                      ("gsr_rcnn_loss", ("scores", "deltas", "rois", "labels", "gt_row", "gtb", "ws", "loss")),
                      ("gsr_rcnn_postprocess", ("scores", "deltas", "prop", "ws", "dets", "counts"))):
        for n in names:
            assert CALLS[fn](lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), (fn, n)
            if n != "ws":
                assert CALLS[fn](lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), (fn, n)
    assert _fwd(lib, cs, n_roi=FAKE, stride=0) == INVALID and b"n_roi_stride" in lib.gsr_last_error()
    assert _bwd(lib, cs, n_roi=FAKE, stride=-2) == INVALID and b"n_roi_stride" in lib.gsr_last_error()
    n = ctypes.c_int64(-1)
    assert lib.gsr_rcnn_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0
    for call in (_loss, _post):
        assert call(lib, cs, ws_bytes=255) == INVALID and b"needed" in lib.gsr_last_error()
        assert call(lib, cs, ws=FAKE + 8) == INVALID and b"16-byte aligned" in lib.gsr_last_error()
    # the loss alone needs less than the output stage; a spec fit for neither is refused
    lo = _spec(R=0, max_det=0)
    m = ctypes.c_int64(-1)
    assert lib.gsr_rcnn_workspace_bytes(ctypes.byref(lo), ctypes.byref(m)) == 0 and 0 < m.value < n.value
    assert _loss(lib, cs, ws_bytes=m.value - 1) == INVALID and _post(lib, cs, ws_bytes=m.value) == INVALID
    bad = _spec(R=0, S=0)
    k = ctypes.c_int64(-1)
    assert lib.gsr_rcnn_workspace_bytes(ctypes.byref(bad), ctypes.byref(k)) == INVALID and k.value == -1
    assert lib.gsr_rcnn_workspace_bytes(ctypes.byref(cs), None) == INVALID


def test_cpu_tensors_raise_and_python_checks():
    prop, gtb, gtc = torch.zeros(2, 6, 4), torch.zeros(2, 1, 4), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.sample(prop, gtb, gtc, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.roi_align(torch.zeros(2, 3, 9, 11), torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.rcnn_loss(torch.zeros(2, 4, 4), torch.zeros(2, 4, 12), torch.zeros(2, 4, 4), torch.zeros(2, 4), torch.zeros(2, 4), gtb)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.postprocess(torch.zeros(2, 4, 4), torch.zeros(2, 4, 12), torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        RD.ProposalSampler(0)
    with pytest.raises(ValueError):
        RD.ProposalSampler(3, per_image=2000)
    with pytest.raises(ValueError):
        RD.RoIHeadLoss(3, cls=-1.0)
    with pytest.raises(ValueError):
        RD.RoIHeadOutput((0.0, 10.0))
    s = RD.ProposalSampler(80)
    assert (s.spec.S, s.spec.max_pos) == (512, 128) and RD.RoIHeadLoss(80).spec.w_box == 0.0
    import gsplat_attack
    assert gsplat_attack.make_roi_loss_fn is RD.make_roi_loss_fn and gsplat_attack.ProposalSampler is RD.ProposalSampler

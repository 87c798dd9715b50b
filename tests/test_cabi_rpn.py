"""The RPN proposal stage's C ABI and Python surface, the parts that need no GPU: symbols, the capability bit in a new
item next to the closed ones, the struct layout, every argument check (refused before any device call: the pointers handed
over are never followed), the workspace size, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import rpn_ops as PO
from gsplat_attack import proposals as PP

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return PO._lib()


def _spec(**kw):
    cs = PO.c_spec(PO.RpnSpec(img_w=640.0, img_h=480.0, pre_topk=100, post_topk=50, iou_thr=0.7), B=2, A=3, Hf=9, Wf=11, stride=16,
                   level=0, cand_offset=20, N=128)
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


def _ref(cs):
    return ctypes.byref(cs) if cs is not None else None


def _select(lib, cs, logits=FAKE, deltas=FAKE, cell=FAKE, cb=FAKE, csc=FAKE, cl=FAKE):
    return lib.gsr_rpn_select(_ref(cs), logits, deltas, cell, cb, csc, cl, None)


def _nms(lib, cs, cb=FAKE, csc=FAKE, cl=FAKE, ws=FAKE, ws_bytes=BIG, prop=FAKE, scores=FAKE, keep=FAKE, counts=FAKE):
    return lib.gsr_rpn_nms(_ref(cs), cb, csc, cl, ws, ws_bytes, prop, scores, keep, counts, None)


CALLS = {"gsr_rpn_select": _select, "gsr_rpn_nms": _nms}


def test_symbols_version_and_capability(lib):
    for name, n in (("gsr_rpn_workspace_bytes", 2), ("gsr_rpn_select", 8), ("gsr_rpn_nms", 11)):
        assert len(getattr(lib, name).argtypes) == n
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(3, ctypes.byref(out)) == 0 and out.value == 15          # closed at bits 0..3
    assert lib.gsr_query(4, ctypes.byref(out)) == 0 and out.value == 31          # closed at bits 0..4
    assert lib.gsr_query(5, ctypes.byref(out)) == 0 and out.value == 63          # every capability bit
    assert lib.gsr_query(6, ctypes.byref(out)) == INVALID
    assert PO.available() and PO.GSR_CAP_RPN == 32
    names = [f[0] for f in PO._CRpnSpec._fields_]
    assert names == ["B", "A", "Hf", "Wf", "stride", "shift0", "img_w", "img_h", "min_size", "pre_topk", "level", "cand_offset", "N",
                     "post_topk", "iou_thr", "flags"]
    assert ctypes.sizeof(PO._CRpnSpec) == 4 * len(names) == 64
    assert [getattr(PO._CRpnSpec, n).offset for n in names] == list(range(0, 64, 4))
    d = PO.RpnSpec()
    assert (d.pre_topk, d.post_topk, d.iou_thr, d.min_size) == (12000, 2000, 0.7, 0.0)
    assert (PO.MAX_SLOTS, PO.MAX_POST) == (16384, 4096)


BAD = {
    "gsr_rpn_select": [dict(B=0), dict(B=65536), dict(flags=1), dict(A=0), dict(Hf=0), dict(Wf=-1), dict(stride=0), dict(N=0), dict(N=16385),
                       dict(shift0=NAN), dict(shift0=INF), dict(img_w=0.0), dict(img_h=NAN), dict(img_h=-4.0), dict(img_w=INF),
                       dict(min_size=-1.0), dict(min_size=NAN), dict(pre_topk=0), dict(level=-1), dict(cand_offset=-1),
                       dict(cand_offset=29),                      # 29 + min(100, 297) > 128
                       dict(pre_topk=109), dict(Hf=1, Wf=1, pre_topk=3, cand_offset=126),     # 20 + 109 > 128; 126 + 3 > 128
                       dict(A=4096, Hf=1024, Wf=1024), dict(Hf=1 << 20, Wf=1, stride=32)],
    "gsr_rpn_nms": [dict(B=0), dict(flags=0x80000000), dict(N=0), dict(N=16385), dict(post_topk=0), dict(post_topk=129),
                    dict(N=8192, post_topk=4097), dict(iou_thr=NAN), dict(iou_thr=-0.1), dict(iou_thr=INF)],
}


@pytest.mark.parametrize("fn", sorted(BAD))
def test_spec_checks(lib, fn):
    for bad in BAD[fn]:                                    # (a valid spec is never sent with the fake pointers)
        assert CALLS[fn](lib, _spec(**bad)) == INVALID, (fn, bad)
        assert fn.encode() + b":" in lib.gsr_last_error(), (fn, bad)
    assert CALLS[fn](lib, None) == INVALID and b"null spec" in lib.gsr_last_error()


def test_the_slot_range_may_end_at_n(lib):
    """cand_offset + min(pre_topk, A*Hf*Wf) == N passes the spec check: what is refused next is the null pointer."""
    for ok in (dict(cand_offset=28), dict(pre_topk=108), dict(Hf=1, Wf=1, pre_topk=5000, cand_offset=125), dict(N=16384, post_topk=4096)):
        assert _select(lib, _spec(**ok), logits=None) == INVALID and b"null logits" in lib.gsr_last_error(), ok
    assert _nms(lib, _spec(N=16384, post_topk=4096), cb=None) == INVALID and b"null cand_boxes" in lib.gsr_last_error()


def test_null_and_misaligned_pointers_and_workspaces(lib):
    cs = _spec()
    for fn, names in (("gsr_rpn_select", ("logits", "deltas", "cell", "cb", "csc", "cl")),
                      ("gsr_rpn_nms", ("cb", "csc", "cl", "ws", "prop", "scores", "keep", "counts"))):
        for n in names:
            assert CALLS[fn](lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), (fn, n)
            if n != "ws":
                assert CALLS[fn](lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), (fn, n)
    n = ctypes.c_int64(-1)
    assert lib.gsr_rpn_workspace_bytes(ctypes.byref(cs), ctypes.byref(n)) == 0 and n.value >= 2 * 128 * 4 and n.value % 256 == 0
    assert _nms(lib, cs, ws_bytes=n.value - 1) == INVALID and b"needed" in lib.gsr_last_error()
    assert _nms(lib, cs, ws=FAKE + 8) == INVALID and b"16-byte aligned" in lib.gsr_last_error()
    k = ctypes.c_int64(-1)
    assert lib.gsr_rpn_workspace_bytes(ctypes.byref(_spec(N=0)), ctypes.byref(k)) == INVALID and k.value == -1
    assert lib.gsr_rpn_workspace_bytes(ctypes.byref(cs), None) == INVALID
    assert lib.gsr_rpn_workspace_bytes(None, ctypes.byref(k)) == INVALID


def test_cpu_tensors_raise_and_python_checks():
    lg, dl, ca = torch.zeros(2, 3, 4, 5), torch.zeros(2, 12, 4, 5), torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        PO.select(lg, dl, ca, 16, PO.RpnSpec(), PO.new_candidates(2, 60, "cpu"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PO.nms(torch.zeros(2, 8, 4), torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32), PO.RpnSpec())
    with pytest.raises(RuntimeError, match="no CPU path"):
        PO.propose([PO.Level(lg, dl, ca, 16)], PO.RpnSpec())
    prop = PP.RpnProposer([(ca, 16, 0.0)], (80.0, 64.0))
    assert (prop.spec.pre_topk, prop.spec.post_topk, prop.spec.iou_thr, prop.spec.min_size) == (12000, 2000, 0.7, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        prop.propose(lg, dl)
    with pytest.raises(RuntimeError, match="head"):
        prop(torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError):
        prop.propose([lg, lg], [dl, dl])
    for bad in (dict(frame=(0.0, 10.0)), dict(post_topk=4097), dict(pre_topk=0), dict(pre_topk=16385), dict(nms=-0.5), dict(min_size=NAN)):
        kw = dict(frame=(80.0, 64.0))
        kw.update(bad)
        with pytest.raises(ValueError):
            PP.RpnProposer([(ca, 16, 0.0)], **kw)
    with pytest.raises(ValueError):
        PP.RpnProposer([], (80.0, 64.0))
    with pytest.raises(ValueError):
        PP.RpnProposer([(torch.zeros(3, 5), 16, 0.0)], (80.0, 64.0))
    import gsplat_attack
    assert gsplat_attack.RpnProposer is PP.RpnProposer and gsplat_attack.cell_anchors is PP.cell_anchors

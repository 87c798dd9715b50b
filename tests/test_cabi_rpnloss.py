"""The RPN loss stage's C ABI and Python surface, the parts that need no GPU: the three symbols and their signatures, the
struct layout, every argument check (refused before any device call: the pointers handed over are never followed), the
version, capability and query items left as they were, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import _signatures as SG
from diff_gaussian_rasterization import rpnloss_ops as RO
from gsplat_attack import proposals as PR
from gsplat_attack import roi_detector as RD

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
NAN, INF = float("nan"), float("inf")
LEVELS = ((3, 50, 68, 4, 0.0), (3, 25, 34, 8, 0.0), (3, 13, 17, 16, 8.0))       # (A, Hf, Wf, stride, shift0)


@pytest.fixture(scope="module")
def lib():
    return RO._lib()


def _spec(**kw):
    cs = RO.c_spec(RO.RpnLossSpec(), B=2, M=3, levels=LEVELS)
    for k, v in kw.items():
        if isinstance(v, dict):                      # an element of an array member: {index: value}
            for i, e in v.items():
                getattr(cs, k)[i] = e
        else:
            setattr(cs, k, v)
    return cs


def _ref(cs):
    return ctypes.byref(cs) if cs is not None else None


def _levels(n=5):
    """A host array of level pointers."""
    return (ctypes.c_void_p * n)(*([FAKE] * n))


BIG = 1 << 40


def _ws_bytes(lib, cs):
    n = ctypes.c_int64(0)
    assert lib.gsr_rpnloss_workspace_bytes(_ref(cs), ctypes.byref(n)) == 0
    return n.value


def _size(lib, cs):
    return lib.gsr_rpnloss_workspace_bytes(_ref(cs), ctypes.byref(ctypes.c_int64(0)))


def _label(lib, cs, cells="all", gt=FAKE, cls=FAKE, ws=FAKE, ws_bytes=BIG, labels=FAKE, matched=FAKE, counts=FAKE, pre=FAKE):
    return lib.gsr_rpnloss_label(_ref(cs), _levels() if cells == "all" else cells, gt, cls, ws, ws_bytes, labels, matched, counts, pre, None)


def _loss(lib, cs, labels=FAKE, matched=FAKE, logits="all", deltas="all", cells="all", gt=FAKE, ws=FAKE, ws_bytes=BIG, loss=FAKE,
          gl="all", gd="all"):
    arr = lambda v: _levels() if v == "all" else v
    return lib.gsr_rpnloss(_ref(cs), labels, matched, arr(logits), arr(deltas), arr(cells), gt, ws, ws_bytes, loss, arr(gl), arr(gd), None)


CALLS = {"gsr_rpnloss_workspace_bytes": _size, "gsr_rpnloss_label": _label, "gsr_rpnloss": _loss}


def test_symbols_signatures_version_and_capability(lib):
    assert RO.available()
    for name, n in (("gsr_rpnloss_workspace_bytes", 2), ("gsr_rpnloss_label", 11), ("gsr_rpnloss", 13)):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == list(SG.SIGNATURES[name][1]) and len(SG.SIGNATURES[name][1]) == n
        assert getattr(lib, name).restype is SG.SIGNATURES[name][0] is ctypes.c_int
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    for item, value in ((3, 15), (4, 31), (5, 63)):
        assert lib.gsr_query(item, ctypes.byref(out)) == 0 and out.value == value
    assert lib.gsr_query(6, ctypes.byref(out)) == INVALID
    names = [f[0] for f in RO._CRpnLossSpec._fields_]
    assert names == ["B", "M", "nl", "A", "Hf", "Wf", "stride", "shift0", "batch_per_image", "pos_quota", "seed", "iou_lo", "iou_hi",
                     "beta", "w_cls", "w_loc", "flags"]
    assert ctypes.sizeof(RO._CRpnLossSpec) == 4 * (3 + 5 * 5 + 9) == 148
    assert [getattr(RO._CRpnLossSpec, n).offset for n in names] == [0, 4, 8, 12, 32, 52, 72, 92, 112, 116, 120, 124, 128, 132, 136, 140, 144]
    d = RO.RpnLossSpec()
    assert (d.batch_per_image, d.pos_quota, d.iou_lo, d.iou_hi, d.beta, d.w_cls, d.w_loc) == (256, 128, 0.3, 0.7, 0.0, 1.0, 1.0)
    assert (RO.MAX_LEVELS, RO.MAX_ROWS, RO.MAX_ANCHORS) == (5, 256, 1 << 24)


def test_workspace_grows_with_the_anchors(lib):
    small, large = _ws_bytes(lib, _spec()), _ws_bytes(lib, _spec(B=4))
    R = sum(a * h * w for a, h, w, _, _ in LEVELS)
    assert small >= 2 * R * 4 and large >= 4 * R * 4 and large > small and small % 256 == 0
    assert lib.gsr_rpnloss_workspace_bytes(_ref(_spec()), None) == INVALID and b"null bytes" in lib.gsr_last_error()


BAD = [dict(B=0), dict(B=65536), dict(M=0), dict(M=257), dict(nl=0), dict(nl=6), dict(nl=-1), dict(flags=1),
       dict(A={0: 0}), dict(Hf={1: 0}), dict(Wf={2: -3}), dict(stride={0: 0}), dict(stride={1: -8}), dict(stride={2: 1 << 21}),
       dict(shift0={0: NAN}), dict(shift0={2: INF}), dict(shift0={1: -INF}),
       dict(batch_per_image=0), dict(batch_per_image=65537), dict(pos_quota=-1), dict(pos_quota=257),
       dict(iou_lo=NAN), dict(iou_hi=NAN), dict(iou_lo=-0.1), dict(iou_hi=INF), dict(iou_lo=0.8),                       # lo above hi
       dict(beta=-1.0), dict(beta=NAN), dict(beta=INF), dict(w_cls=-1.0), dict(w_cls=NAN), dict(w_loc=INF), dict(w_loc=-0.5),
       dict(A={0: 1 << 20}, Hf={0: 4}, Wf={0: 8}),                                   # a level beyond 2^24 anchors
       dict(Hf={0: 1 << 16}, Wf={0: 1 << 16}),                                       # ... by its cells alone (no overflow on the way)
       dict(A={0: 0x7fffffff}, Hf={0: 0x7fffffff}, Wf={0: 0x7fffffff}),
       dict(nl=5, A={l: 5 for l in range(5)}, Hf={l: 1024 for l in range(5)}, Wf={l: 1024 for l in range(5)}, stride={l: 1 for l in range(5)},
            shift0={l: 0.0 for l in range(5)}),                                      # every level within 2^24, the sum beyond
       dict(B=200, A={0: 12}, Hf={0: 1024}, Wf={0: 1024}, stride={0: 1}),           # B * R beyond 2^31 - 1
       dict(B=60, A={0: 9}, Hf={0: 1024}, Wf={0: 1024}, stride={0: 1}),             # a deltas tensor beyond 2^31 - 1 elements
       ]


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_spec_checks(lib, fn):
    for bad in BAD:                                        # (a valid spec is never sent with the fake pointers)
        assert CALLS[fn](lib, _spec(**bad)) == INVALID, (fn, bad)
        assert fn.encode() + b":" in lib.gsr_last_error(), (fn, bad)
    assert CALLS[fn](lib, None) == INVALID and b"null spec" in lib.gsr_last_error()


def test_null_misaligned_pointers_and_workspace(lib):
    cs = _spec()
    need = _ws_bytes(lib, cs)
    for n in ("gt", "cls", "ws", "labels", "matched", "counts"):
        assert _label(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
    for n in ("gt", "cls", "labels", "matched", "counts", "pre"):
        assert _label(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    assert _label(lib, cs, cells=None) == INVALID and b"null" in lib.gsr_last_error()
    for n in ("labels", "matched", "gt", "ws", "loss", "logits", "deltas", "cells"):
        assert _loss(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
    for n in ("labels", "matched", "gt", "loss"):
        assert _loss(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    for call in (_label, _loss):
        assert call(lib, cs, ws_bytes=need - 1) == INVALID and b"gsr_rpnloss_workspace_bytes" in lib.gsr_last_error()
        assert call(lib, cs, ws_bytes=0) == INVALID
        assert call(lib, cs, ws=FAKE + 8) == INVALID and b"16-byte aligned" in lib.gsr_last_error()
    for l in range(3):                                      # every one of the nl level pointers of every array
        for call, names in ((_label, ("cells",)), (_loss, ("logits", "deltas", "cells", "gl", "gd"))):
            for n in names:
                a = _levels()
                a[l] = None
                assert call(lib, cs, **{n: a}) == INVALID and b"level %d" % l in lib.gsr_last_error(), (n, l)
                a[l] = FAKE + 2
                assert call(lib, cs, **{n: a}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), (n, l)
    a = _levels()
    a[3] = a[4] = None                                      # beyond nl: not read
    assert _label(lib, cs, cells=a, gt=None) == INVALID and b"null cell_anchors / gt_boxes" in lib.gsr_last_error()
    assert _loss(lib, cs, logits=a, deltas=a, cells=a, gl=a, gd=a, loss=None) == INVALID and b"/ loss" in lib.gsr_last_error()


def test_cpu_tensors_raise_and_python_checks():
    ca = torch.tensor([[-16.0, -16.0, 16.0, 16.0]])
    lv = [RO.AnchorLevel(ca, 16, (5, 7))]
    gt, cls = torch.zeros(2, 1, 4), torch.zeros(2, 1, dtype=torch.int32)
    x, d = torch.zeros(2, 1, 5, 7, requires_grad=True), torch.zeros(2, 4, 5, 7)
    lab = torch.zeros(2, 35, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.label(lv, gt, cls, RO.RpnLossSpec())
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.loss_forward([x], [d], lv, lab, lab, gt, RO.RpnLossSpec())
    with pytest.raises(RuntimeError, match="no CPU path"):
        RO.rpn_loss([x], [d], lv, gt, cls)
    rl = PR.RpnLoss([(ca, 16)], batch_per_image=8, positive_fraction=0.5, iou=(0.25, 0.5), cls=2.0, loc=0.5, beta=0.1, seed=9)
    assert rl.spec == RO.RpnLossSpec(batch_per_image=8, pos_quota=4, seed=9, iou_lo=0.25, iou_hi=0.5, beta=0.1, w_cls=2.0, w_loc=0.5)
    assert PR.RpnLoss([(ca, 16)]).spec == RO.RpnLossSpec() and PR.RpnLoss([(ca, 16)], batch_per_image=7).spec.pos_quota == 3
    with pytest.raises(RuntimeError, match="no CPU path"):
        rl.loss(x, d, gt[:, 0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        rl.labels([(5, 7)], gt)
    with pytest.raises(ValueError):
        rl.loss([x, x], [d, d], gt)
    for bad in (dict(levels=[]), dict(levels=[(ca, 16)] * 6), dict(levels=[(ca, 0)]), dict(levels=[(ca[:, :3], 16)]), dict(batch_per_image=0),
                dict(positive_fraction=1.5), dict(iou=(0.7, 0.3)), dict(iou=(-0.1, 0.5)), dict(cls=-1.0), dict(loc=INF), dict(beta=NAN)):
        with pytest.raises(ValueError):
            PR.RpnLoss(**{"levels": [(ca, 16)], **bad})
    with pytest.raises(ValueError, match="rpn_loss needs a proposer"):
        RD.make_roi_loss_fn(lambda x: x, lambda f: f, lambda p: p, None, RD.ProposalSampler(2), RD.RoIHeadLoss(2), torch.zeros(1, 4), 0, rpn_loss=rl)
    import gsplat_attack
    assert gsplat_attack.RpnLoss is PR.RpnLoss

"""The FPN RoI pooler's C ABI and Python surface, the parts that need no GPU: both symbols and their signatures, the struct
layout, every argument check (refused before any device call: the pointers handed over are never followed), the capability
items left as they were, and CPU tensors (no fallback)."""
import ctypes

import pytest
import torch

from diff_gaussian_rasterization import _signatures as SG
from diff_gaussian_rasterization import fpn_ops as FO
from gsplat_attack import roi_detector as RD

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
NAN, INF = float("nan"), float("inf")
SIZES = ((97, 125), (49, 63), (25, 32), (13, 16))


@pytest.fixture(scope="module")
def lib():
    return FO._lib()


def _spec(**kw):
    cs = FO.c_spec(FO.FpnSpec(), B=2, S=24, Cf=3, sizes=SIZES)
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


def _fwd(lib, cs, feats="all", rois=FAKE, n_roi=FAKE, stride=2, pooled=FAKE, lv=FAKE, ll=FAKE, lc=FAKE):
    return lib.gsr_fpn_pool(_ref(cs), _levels() if feats == "all" else feats, rois, n_roi, stride, pooled, lv, ll, lc, None)


def _bwd(lib, cs, rois=FAKE, ll=FAKE, lc=FAKE, gp=FAKE, grads="all", acc=0):
    return lib.gsr_fpn_pool_backward(_ref(cs), rois, ll, lc, gp, _levels() if grads == "all" else grads, acc, None)


CALLS = {"gsr_fpn_pool": _fwd, "gsr_fpn_pool_backward": _bwd}


def test_symbols_signatures_version_and_capability(lib):
    assert FO.available()
    for name, n in (("gsr_fpn_pool", 10), ("gsr_fpn_pool_backward", 8)):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == list(SG.SIGNATURES[name][1]) and len(SG.SIGNATURES[name][1]) == n
        assert getattr(lib, name).restype is SG.SIGNATURES[name][0] is ctypes.c_int
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    assert lib.gsr_query(5, ctypes.byref(out)) == 0 and out.value == 63
    assert lib.gsr_query(6, ctypes.byref(out)) == INVALID
    names = [f[0] for f in FO._CFpnSpec._fields_]
    assert names == ["B", "S", "Cf", "PH", "PW", "sampling_ratio", "nl", "Hf", "Wf", "scale", "thr", "canonical_size"]
    assert ctypes.sizeof(FO._CFpnSpec) == 4 * (7 + 4 * 5 + 1) == 112
    assert [getattr(FO._CFpnSpec, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28, 48, 68, 88, 108]
    d = FO.FpnSpec()
    assert (d.PH, d.PW, d.sampling_ratio, d.canonical_size, d.thr) == (7, 7, 0, 224.0, (0.0, 0.5, 1.0, 2.0))
    assert FO.level_thresholds((4, 8, 16, 32)) == (0.0, 0.5, 1.0, 2.0) and FO.level_thresholds((8, 16), 4) == (0.0, 1.0)
    assert FO.MAX_LEVELS == 5


BAD = [dict(B=0), dict(B=65536), dict(S=0), dict(S=1025), dict(Cf=0), dict(Cf=65536), dict(PH=0), dict(PH=15), dict(PW=0), dict(PW=15),
       dict(sampling_ratio=-1), dict(nl=0), dict(nl=6), dict(nl=-1), dict(Hf={0: 0}), dict(Wf={3: -2}), dict(scale={1: 0.0}),
       dict(scale={2: NAN}), dict(scale={0: INF}), dict(scale={3: -0.25}),
       dict(thr={1: 0.0}), dict(thr={1: NAN}), dict(thr={3: INF}), dict(thr={2: 0.5}), dict(thr={2: 0.25}), dict(thr={3: 1.0}),    # not ascending
       dict(canonical_size=0.0), dict(canonical_size=NAN), dict(canonical_size=INF), dict(canonical_size=-224.0),
       dict(B=65535, S=1024, Cf=4096),                                        # pooled beyond 2^31 - 1 elements
       dict(B=64, Cf=64, Hf={0: 1024}, Wf={0: 1024}),                       # a level's features beyond 2^31 - 1 elements
       dict(Cf=1, B=1, Hf={0: 46341, 1: 46341, 2: 46341, 3: 46341}, Wf={0: 46341, 1: 46341, 2: 46341, 3: 46341}),    # 46341^2 > 2^31 - 1
       ]
# (the limit of 2^31 - 1 tiles in all cannot be reached by a spec that passes the element limits: a level of at most 2^31 - 1
# cells holds at most 2^28 tiles, five of them 1.25 * 2^30)


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_spec_checks(lib, fn):
    for bad in BAD:                                        # (a valid spec is never sent with the fake pointers)
        assert CALLS[fn](lib, _spec(**bad)) == INVALID, (fn, bad)
        assert fn.encode() + b":" in lib.gsr_last_error(), (fn, bad)
    assert CALLS[fn](lib, None) == INVALID and b"null spec" in lib.gsr_last_error()


def test_null_and_misaligned_pointers(lib):
    cs = _spec()
    for n in ("rois", "pooled", "lv", "ll", "lc"):
        assert _fwd(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
        assert _fwd(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    assert _fwd(lib, cs, n_roi=FAKE + 1) == INVALID and b"4-byte aligned" in lib.gsr_last_error()
    assert _fwd(lib, cs, stride=0) == INVALID and b"n_roi_stride" in lib.gsr_last_error()
    assert _fwd(lib, cs, feats=None) == INVALID and b"null" in lib.gsr_last_error()
    for n in ("rois", "ll", "lc", "gp"):
        assert _bwd(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
        assert _bwd(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    assert _bwd(lib, cs, grads=None) == INVALID and b"null" in lib.gsr_last_error()
    for l in range(4):                                      # every one of the nl level pointers
        a = _levels()
        a[l] = None
        assert _fwd(lib, cs, feats=a) == INVALID and b"level %d" % l in lib.gsr_last_error()
        assert _bwd(lib, cs, grads=a) == INVALID and b"level %d" % l in lib.gsr_last_error()
        a[l] = FAKE + 2
        assert _fwd(lib, cs, feats=a) == INVALID and b"4-byte aligned" in lib.gsr_last_error()
        assert _bwd(lib, cs, grads=a) == INVALID and b"4-byte aligned" in lib.gsr_last_error()
    a = _levels()
    a[4] = None                                             # beyond nl: not read
    assert _fwd(lib, cs, feats=a, rois=None) == INVALID and b"null features / rois" in lib.gsr_last_error()


def test_cpu_tensors_raise_and_python_checks():
    feats = [torch.zeros(2, 3, h, w) for h, w in SIZES]
    rois = torch.zeros(2, 24, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FO.pool_forward(feats, rois, None, FO.FpnSpec())
    with pytest.raises(RuntimeError, match="no CPU path"):
        FO.fpn_pool(feats, rois)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FO.pool_backward(torch.zeros(2, 24, 3, 7, 7), rois, torch.zeros(2, 4, 24, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                         [f.shape for f in feats], FO.FpnSpec())
    pooler = RD.FpnRoIPooler()
    assert pooler.strides == (4, 8, 16, 32) and pooler.spec == FO.FpnSpec()
    with pytest.raises(RuntimeError, match="no CPU path"):
        pooler(feats, rois)
    with pytest.raises(ValueError):
        pooler(feats[:3], rois)
    for bad in (dict(strides=(4, 8, 12)), dict(strides=(4, 16)), dict(strides=(3, 6)), dict(strides=()), dict(strides=(1, 2, 4, 8, 16, 32)),
                dict(output_size=15), dict(output_size=(0, 7)), dict(sampling_ratio=-1), dict(canonical_size=0.0), dict(canonical_size=INF)):
        with pytest.raises(ValueError):
            RD.FpnRoIPooler(**bad)
    p = RD.FpnRoIPooler(strides=(8, 16, 32, 64), output_size=(3, 5), canonical_level=5)
    assert p.spec.thr == (0.0, 0.5, 1.0, 2.0) and (p.spec.PH, p.spec.PW) == (3, 5)
    assert RD.FpnRoIPooler(strides=(16,)).spec.thr == (0.0,)
    import gsplat_attack
    assert gsplat_attack.FpnRoIPooler is RD.FpnRoIPooler

"""The object-map classifier's C ABI and Python surface, the parts that need no GPU: both symbols and their signatures, the
struct layout, every argument check (refused before any device call: the pointers handed over are never followed, and
sentinel-filled host buffers handed over as outputs stay as they were), the capability items left as they were, and what the
Python layer refuses (CPU tensors, a classifier or target that requires grad, wrong shapes)."""
import ctypes

import numpy as np
import pytest
import torch

from diff_gaussian_rasterization import _signatures as SG
from diff_gaussian_rasterization import objmap_ops as OM
from gsplat_attack import objects as GO

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
BIG = 1 << 40
OUTS = ("ids", "conf", "stats", "paint", "terms", "grad")


@pytest.fixture(scope="module")
def lib():
    return OM._lib()


def _spec(**kw):
    cs = OM.c_spec((2, 17, 33), 5, OM.LOSS)
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


def _ref(cs):
    return ctypes.byref(cs) if cs is not None else None


def _call(lib, cs, objmap=FAKE, weight=FAKE, bias=FAKE, target=FAKE, palette=FAKE, ws=FAKE, ws_bytes=BIG, ids=FAKE, conf=FAKE,
          stats=FAKE, paint=FAKE, terms=FAKE, grad=FAKE):
    return lib.gsr_objmap(_ref(cs), objmap, weight, bias, target, palette, ws, ws_bytes, ids, conf, stats, paint, terms, grad, None)


def _bytes(lib, cs):
    n = ctypes.c_int64(-1)
    return lib.gsr_objmap_workspace_bytes(_ref(cs), ctypes.byref(n)), n.value


def test_symbols_signatures_layout_and_capability(lib):
    assert OM.available()
    for name, n in (("gsr_objmap_workspace_bytes", 2), ("gsr_objmap", 15)):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == list(SG.SIGNATURES[name][1]) and len(SG.SIGNATURES[name][1]) == n
        assert getattr(lib, name).restype is SG.SIGNATURES[name][0] is ctypes.c_int
    assert SG.SIGNATURES["gsr_objmap"][1][7] is ctypes.c_int64                   # ws_bytes
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604       # no new version, bit or item
    assert lib.gsr_query(5, ctypes.byref(out)) == 0 and out.value == 63
    assert lib.gsr_query(6, ctypes.byref(out)) == INVALID
    names = [f[0] for f in OM._CObjMapSpec._fields_]
    assert names == ["B", "H", "W", "K", "flags"] and ctypes.sizeof(OM._CObjMapSpec) == 20
    assert [getattr(OM._CObjMapSpec, n).offset for n in names] == [0, 4, 8, 12, 16]
    assert (OM.CHANNELS, OM.MAX_CLASSES, OM.LOSS) == (16, 1024, 1)


BAD = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=-3), dict(K=0), dict(K=-1), dict(K=1025), dict(B=65536),
       dict(B=1, H=46341, W=46341),                                # 46341^2 > 2^31 - 1
       dict(B=8, H=4096, W=4096),                                  # B 16 H W = 2^31
       dict(B=2147483647, H=2147483647, W=2147483647),             # every product overflows 64 bits' lower half
       dict(flags=2), dict(flags=0x80000001)]


def test_spec_checks(lib):
    for bad in BAD:
        assert _call(lib, _spec(**bad)) == INVALID, bad
        assert b"gsr_objmap:" in lib.gsr_last_error(), bad
        rc, _ = _bytes(lib, _spec(**bad))
        assert rc == INVALID and b"gsr_objmap_workspace_bytes:" in lib.gsr_last_error(), bad
    assert _call(lib, None) == INVALID and b"null spec" in lib.gsr_last_error()
    assert lib.gsr_objmap_workspace_bytes(None, ctypes.byref(ctypes.c_int64())) == INVALID and b"null spec" in lib.gsr_last_error()
    assert lib.gsr_objmap_workspace_bytes(_ref(_spec()), None) == INVALID and b"null bytes" in lib.gsr_last_error()


def test_workspace_bytes_and_pointer_checks(lib):
    cs, plain = _spec(), _spec(flags=0)
    rc, full = _bytes(lib, cs)
    rc2, none = _bytes(lib, plain)
    nblk = -(-17 * 33 // 256)
    assert rc == 0 and rc2 == 0 and none == 0 and full >= 4 * 2 * nblk + 4 * 2 * 64 and full % 16 == 0
    for n in ("objmap", "weight", "bias", "ids"):
        assert _call(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
    assert _call(lib, cs, ws=None) == INVALID and b"null ws" in lib.gsr_last_error()
    for n in ("objmap", "weight", "bias", "target", "ids", "conf", "stats", "terms", "grad"):
        assert _call(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    assert _call(lib, cs, ws_bytes=full - 1) == INVALID and b"workspace of" in lib.gsr_last_error()
    assert _call(lib, cs, ws_bytes=0) == INVALID and _call(lib, cs, ws_bytes=-5) == INVALID
    for off in (4, 8, 12):
        assert _call(lib, cs, ws=FAKE + off) == INVALID and b"16-byte aligned" in lib.gsr_last_error(), off
        assert _call(lib, plain, ws=FAKE + off, terms=None, grad=None) == INVALID and b"16-byte aligned" in lib.gsr_last_error(), off
    # paint without a palette; terms or grad without a target, or without the flag
    assert _call(lib, cs, palette=None) == INVALID and b"palette" in lib.gsr_last_error()
    for kw in (dict(grad=None), dict(terms=None)):
        assert _call(lib, cs, target=None, **kw) == INVALID and b"without a target" in lib.gsr_last_error(), kw
        assert _call(lib, plain, **kw) == INVALID and b"GSR_OBJMAP_LOSS" in lib.gsr_last_error(), kw
    # (a call that passes every check is never made with the fake pointers)


def test_refused_calls_leave_the_outputs_alone(lib):
    """Real host buffers this time: had a refused call launched or written anything, the sentinels would show it (or the
    process would have faulted on a host pointer)."""
    B, H, W, K = 2, 17, 33, 5
    bufs = dict(ids=np.full((B, H, W), -7, np.int32), conf=np.full((B, H, W), -7, np.float32), stats=np.full((B, K, 5), -7, np.int32),
                paint=np.full((B, H, W, 3), 7, np.uint8), terms=np.full((B, 2), -7, np.float32), grad=np.full((B, 16, H, W), -7, np.float32))
    before = {k: v.copy() for k, v in bufs.items()}
    ptrs = {k: v.ctypes.data for k, v in bufs.items()}
    refusals = [(_spec(K=0), {}), (_spec(K=1025), {}), (_spec(H=0), {}), (_spec(B=8, H=4096, W=4096), {}), (_spec(), dict(palette=None)),
                (_spec(), dict(target=None)), (_spec(flags=0), {}), (_spec(), dict(ws_bytes=16)), (_spec(), dict(ws=FAKE + 8)),
                (_spec(), dict(objmap=FAKE + 1))]
    for cs, kw in refusals:
        args = dict(ptrs)
        args.update(kw)
        assert _call(lib, cs, **args) == INVALID and lib.gsr_last_error(), (kw, cs.K, cs.H)
    for k in OUTS:
        assert bufs[k].tobytes() == before[k].tobytes(), k


def test_python_layer_refuses_without_a_device():
    x, w, b = torch.rand(1, 16, 6, 7), torch.rand(5, 16), torch.rand(5)
    t = torch.zeros(1, 6, 7, dtype=torch.int64)
    clf = GO.ObjectClassifier(5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        OM.objmap_forward(x, w, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        OM.object_ce(x, w, b, t)
    for fn in (lambda: GO.segment_objects(x, clf), lambda: GO.segment_objects(x[0], (w, b), conf=True, paint=True),
               lambda: GO.object_ce(x, t, clf.conv)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    for bad in (dict(weight=w.clone().requires_grad_(True)), dict(bias=b.clone().requires_grad_(True))):
        kw = dict(weight=w, bias=b)
        kw.update(bad)
        with pytest.raises(ValueError, match="must not require grad"):
            OM.object_ce(x, kw["weight"], kw["bias"], t)
        with pytest.raises(ValueError, match="must not require grad"):
            OM.objmap_forward(x, kw["weight"], kw["bias"])
    with pytest.raises(TypeError):
        GO.segment_objects(x, object())
    with pytest.raises(ValueError):
        GO.classifier_parameters(torch.nn.Conv2d(16, 5, 3))
    wt, bs = GO.classifier_parameters(clf)
    assert tuple(wt.shape) == (5, 16) and tuple(bs.shape) == (5,) and not wt.requires_grad
    pal = GO.object_palette(300)
    assert pal.dtype == torch.uint8 and tuple(pal.shape) == (300, 3) and not pal[0].any()
    assert all(np.array_equal(pal[i].numpy(), GO.id2rgb(i)) for i in (1, 7, 255, 256))
    import gsplat_attack
    for n in ("segment_objects", "object_boxes", "group_bboxes", "object_ce", "ObjectMaps"):
        assert getattr(gsplat_attack, n) is getattr(GO, n)


def test_object_boxes_on_the_cpu():
    stats = torch.zeros(2, 4, 5, dtype=torch.int32)
    stats[0, 1] = torch.tensor([6, 2, 3, 5, 5])
    stats[0, 3] = torch.tensor([2, 4, 1, 6, 2])
    stats[1, 1] = torch.tensor([1, 0, 0, 1, 1])
    assert GO.object_boxes(stats, [1, 3]) == [((2, 1, 6, 5), 8), ((0, 0, 1, 1), 1)]
    assert GO.object_boxes(stats, [0, 2]) == [(None, 0), (None, 0)]
    assert GO.object_boxes(stats[0], [3, 3]) == ((4, 1, 6, 2), 2)
    with pytest.raises(ValueError):
        GO.object_boxes(stats, [4])
    with pytest.raises(ValueError):
        GO.object_boxes(stats[0, 0], [0])

"""gsr_knn_query and gsr_knn_gather_mean at the C ABI, without a device: both symbols exist with the table's signatures, every
refusal of include/gsraster.h is made before the first device call (the pointers are fakes that are never followed), and the
version and the capability items are what they were -- the stage is present iff the library exports its symbols."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
FAKE = ctypes.c_void_p(0x1000)            # never followed: every call below is refused or has nothing to do


@pytest.fixture(scope="module")
def lib():
    import diff_gaussian_rasterization as D
    if not os.path.exists(D.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return D._load()


def test_symbols_signatures_version_and_capability(lib):
    from diff_gaussian_rasterization import _signatures as SG, knn_ops
    assert knn_ops.available()
    for name, n in (("gsr_knn_query", 9), ("gsr_knn_gather_mean", 9)):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == list(SG.SIGNATURES[name][1]) and len(SG.SIGNATURES[name][1]) == n
        assert getattr(lib, name).restype is SG.SIGNATURES[name][0] is ctypes.c_int
    assert SG.SIGNATURES["gsr_knn_query"][1][:6] == (SG.PTR, SG.I32, SG.PTR, SG.I32, SG.I32, SG.U32)
    assert SG.SIGNATURES["gsr_knn_gather_mean"][1][:5] == (SG.PTR, SG.I32, SG.I32, SG.I32, SG.I32)
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604           # no new version ...
    for item, value in ((3, 15), (4, 31), (5, 63)):                                # ... no new capability bit ...
        assert lib.gsr_query(item, ctypes.byref(out)) == 0 and out.value == value
    assert lib.gsr_query(6, ctypes.byref(out)) == INVALID                          # ... and no new item
    assert (knn_ops.MAX_K, knn_ops.MAX_TENSORS, knn_ops.MAX_COLS, knn_ops.EXCLUDE_SAME_INDEX) == (8, 8, 128, 1)
    header = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    assert "#define GSR_KNNQ_EXCLUDE_SAME_INDEX 1u" in header


def _query(lib, ref=FAKE, R=10, qry=FAKE, Q=10, k=5, flags=0, out_idx=FAKE, out_d2=FAKE):
    return lib.gsr_knn_query(ref, R, qry, Q, k, flags, out_idx, out_d2, None)


@pytest.mark.parametrize("kw, word", [
    (dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(k=-1), b"k=-1"),
    (dict(R=-1), b"R=-1"), (dict(Q=-1), b"Q=-1"),
    (dict(ref=None), b"null"), (dict(qry=None), b"null"), (dict(out_idx=None), b"null"),
    (dict(flags=2), b"flags"), (dict(flags=0x80000000), b"flags"), (dict(flags=3), b"flags"),
    (dict(flags=1, Q=9), b"self-query"), (dict(flags=1, R=0, Q=1), b"self-query"),
])
def test_query_refusals(lib, kw, word):
    assert _query(lib, **kw) == INVALID
    assert word in lib.gsr_last_error(), lib.gsr_last_error()


def test_query_with_no_query_does_nothing(lib):
    assert _query(lib, Q=0, qry=None, out_idx=None, out_d2=None) == 0               # Q = 0 writes nothing
    assert _query(lib, Q=0, R=0, ref=None, qry=None, out_idx=None, out_d2=None) == 0
    assert _query(lib, Q=0, R=0, ref=None, qry=None, out_idx=None, out_d2=None, flags=1) == 0   # the empty self-query


def _arrays(n, cols):
    src = (ctypes.c_void_p * max(n, 1))(*([FAKE.value] * max(n, 1)))
    dst = (ctypes.c_void_p * max(n, 1))(*([FAKE.value] * max(n, 1)))
    col = (ctypes.c_int32 * max(len(cols), 1))(*cols)
    return src, col, dst


def _gather(lib, idx=FAKE, Q=10, k=5, R=10, cols=(3, 45), n=None, src="ok", col="ok", dst="ok"):
    n = len(cols) if n is None else n
    s, c, d = _arrays(len(cols), cols)
    pick = lambda v, a: a if v == "ok" else v
    return lib.gsr_knn_gather_mean(idx, Q, k, R, n, pick(src, s), pick(col, c), pick(dst, d), None)


@pytest.mark.parametrize("kw, word", [
    (dict(k=0), b"k=0"), (dict(k=9), b"k=9"),
    (dict(R=-1), b"R=-1"), (dict(Q=-1), b"Q=-1"),
    (dict(n=0), b"tensors"), (dict(n=9, cols=(1,) * 9), b"tensors"),
    (dict(src=None), b"null"), (dict(col=None), b"null"), (dict(dst=None), b"null"), (dict(idx=None), b"null"),
    (dict(cols=(3, 0)), b"columns"), (dict(cols=(129,)), b"columns"), (dict(cols=(-4,)), b"columns"),
    (dict(cols=(64, 64, 1)), b"columns in all"), (dict(cols=(128, 1)), b"columns in all"),
])
def test_gather_mean_refusals(lib, kw, word):
    assert _gather(lib, **kw) == INVALID
    assert word in lib.gsr_last_error(), lib.gsr_last_error()


def test_gather_mean_null_tensor_pointer_and_empty_call(lib):
    s, c, d = _arrays(2, (3, 4))
    s[1] = None
    assert lib.gsr_knn_gather_mean(FAKE, 10, 5, 10, 2, s, c, d, None) == INVALID and b"tensor 1" in lib.gsr_last_error()
    s, c, d = _arrays(2, (3, 4))
    d[0] = None
    assert lib.gsr_knn_gather_mean(FAKE, 10, 5, 10, 2, s, c, d, None) == INVALID and b"tensor 0" in lib.gsr_last_error()
    assert _gather(lib, Q=0, idx=None, cols=(64, 64)) == 0                         # Q = 0 writes nothing; 128 columns are allowed
    assert _gather(lib, Q=0, idx=None, cols=(64, 65)) == INVALID                   # ... and the checks still run

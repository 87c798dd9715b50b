"""The batch entry points with object channels (C ABI 602): exported, and their argument checks answer before any device
call (this file runs without a GPU)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsr_forward_raw_batch_obj", "gsr_forward_raw2_batch_obj", "gsr_backward_raw_batch_obj_into",
       "gsr_backward_raw_batch_obj_views")
GSR_ERR_INVALID, GSR_ERR_STATE = 1, 4
GSR_FLAG_NEEDLE_DOUBLE = 1 << 20


@pytest.fixture(scope="module")
def lib():
    import diff_gaussian_rasterization as D
    if not os.path.exists(D.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    return D._load()


def _settings(n, flags=0):
    import diff_gaussian_rasterization as D
    arr = (D._CSettings * n)()
    for v in range(n):
        arr[v] = D._CSettings(16, 16, 0.5, 0.5, 8, 1.0, 8, 8, 3, 8, 0, 0, flags)
    return arr


def test_symbols_exported_and_version(lib):
    for n in NEW:
        assert hasattr(lib, n), n
    text = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    for n in NEW:
        assert n + "(" in text, f"{n} not declared in include/gsraster.h"
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value >= 602


def test_forward_batch_obj_argument_checks(lib):
    one = ctypes.c_void_p(8)
    f = lib.gsr_forward_raw_batch_obj
    for B in (0, 17):
        st = _settings(1)
        rc = f(st, B, 4, one, one, one, one, one, one, one, one, one, one, None, None, None)
        assert rc == GSR_ERR_INVALID and b"gsr_forward_raw_batch_obj" in lib.gsr_last_error() and b"views" in lib.gsr_last_error()
    st = _settings(2)
    rc = f(st, 2, 4, one, one, one, None, one, one, one, one, one, one, None, None, None)
    assert rc == GSR_ERR_INVALID
    msg = lib.gsr_last_error()
    assert b"gsr_forward_raw_batch_obj" in msg and b"objects_dc" in msg
    st = _settings(2, GSR_FLAG_NEEDLE_DOUBLE)
    rc = f(st, 2, 4, one, one, one, one, one, one, one, one, one, one, None, None, None)
    assert rc == GSR_ERR_INVALID and b"NEEDLE_DOUBLE" in lib.gsr_last_error()
    # views that disagree in image size
    st = _settings(2)
    st[1].image_width = 32
    rc = f(st, 2, 4, one, one, one, one, one, one, one, one, one, one, None, None, None)
    assert rc == GSR_ERR_INVALID and b"differs from view 0" in lib.gsr_last_error()


def test_forward_pair_batch_obj_argument_checks(lib):
    one = ctypes.c_void_p(8)
    f = lib.gsr_forward_raw2_batch_obj
    a = [one] * 7
    for B in (0, 17):
        rc = f(_settings(1), B, 4, *a, 4, *a, one, one, one, None, None, None)
        assert rc == GSR_ERR_INVALID and b"gsr_forward_raw2_batch_obj" in lib.gsr_last_error()
    # objects: both segments or neither
    b = list(a)
    b[3] = None
    rc = f(_settings(2), 2, 4, *a, 4, *b, one, one, one, None, None, None)
    assert rc == GSR_ERR_INVALID and b"objects_dc" in lib.gsr_last_error()
    rc = f(_settings(2, GSR_FLAG_NEEDLE_DOUBLE), 2, 4, *a, 4, *a, one, one, one, None, None, None)
    assert rc == GSR_ERR_INVALID and b"NEEDLE_DOUBLE" in lib.gsr_last_error()


def test_backward_batch_obj_null_context(lib):
    one = ctypes.c_void_p(8)
    rc = lib.gsr_backward_raw_batch_obj_into(None, one, one, one, None, one, one, one, one, one, one, 0, None)
    assert rc == GSR_ERR_STATE and b"null context" in lib.gsr_last_error()
    rc = lib.gsr_backward_raw_batch_obj_views(None, one, one, one, None, one, one, one, one, one, one, 59 * 4, None)
    assert rc == GSR_ERR_STATE and b"null context" in lib.gsr_last_error()

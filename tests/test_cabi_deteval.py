"""The detection metrics' C ABI and binding, the parts that need no GPU: the four symbols and their signatures, the struct
layout, every limit and every NULL refused before any device call (the pointers handed over are never followed), the version and
the capability items left as they were, and CPU tensors (no fallback)."""
import ctypes

import numpy as np
import pytest
import torch

from diff_gaussian_rasterization import _signatures as SG
from diff_gaussian_rasterization import deteval_ops as EO

INVALID = 1
FAKE = 0x1000          # a non-null, 16-byte aligned pointer that is never followed: every call below is refused first
NAN = float("nan")
COCO = EO.EvalSpec(80, tuple(np.linspace(0.5, 0.95, 10).tolist()), ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10)), (1, 10, 100), 101)


@pytest.fixture(scope="module")
def lib():
    return EO._lib()


def _spec(**kw):
    cs = EO.c_spec(COCO, D=100, M=5)
    for k, v in kw.items():
        if isinstance(v, dict):                      # an element of an array member: {index: value}
            for i, e in v.items():
                getattr(cs, k)[i] = e
        else:
            setattr(cs, k, v)
    return cs


def _ref(cs):
    return ctypes.byref(cs) if cs is not None else None


MATCH_PTRS = ("dets", "counts", "gt_boxes", "gt_cls", "dt_order", "dt_rank", "dt_match", "dt_ignore", "gt_ignore", "gt_match")
ACC_IN = ("dets", "dt_order", "dt_rank", "dt_match", "dt_ignore", "gt_cls", "gt_ignore", "rec_thrs")
ACC_OUT = ("precision", "scores", "recall", "npig")


def _match(lib, cs, B=2, **p):
    return lib.gsr_deteval_match(_ref(cs), B, *[p.get(n, FAKE) for n in MATCH_PTRS], None)


def _acc(lib, cs, N=2, ws=FAKE, ws_bytes=1 << 40, **p):
    return lib.gsr_deteval_accumulate(_ref(cs), N, *[p.get(n, FAKE) for n in ACC_IN], ws, ws_bytes, *[p.get(n, FAKE) for n in ACC_OUT], None)


def _sum(lib, cs, precision=FAKE, recall=FAKE, stats=FAKE):
    return lib.gsr_deteval_summarize(_ref(cs), precision, recall, stats, None)


def _bytes(lib, cs, N=2, out="int"):
    n = ctypes.c_int64(-1)
    return lib.gsr_deteval_workspace_bytes(_ref(cs), N, ctypes.byref(n) if out == "int" else out)


CALLS = {"gsr_deteval_match": _match, "gsr_deteval_accumulate": _acc, "gsr_deteval_summarize": _sum, "gsr_deteval_workspace_bytes": _bytes}


def test_symbols_signatures_version_and_layout(lib):
    assert EO.available()
    for name, n in (("gsr_deteval_workspace_bytes", 3), ("gsr_deteval_match", 13), ("gsr_deteval_accumulate", 17), ("gsr_deteval_summarize", 5)):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == list(SG.SIGNATURES[name][1]) and len(SG.SIGNATURES[name][1]) == n
        assert getattr(lib, name).restype is SG.SIGNATURES[name][0] is ctypes.c_int
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value == 604
    seen = []
    for item in (3, 4, 5):
        assert lib.gsr_query(item, ctypes.byref(out)) == 0
        seen.append(out.value)
    assert seen == [15, 31, 63] and lib.gsr_query(6, ctypes.byref(out)) == INVALID      # no new item, no new bit
    names = [f[0] for f in EO._CDetEvalSpec._fields_]
    assert names == ["K", "D", "M", "T", "A", "n_caps", "max_dets", "R", "iou_thrs", "area_lo", "area_hi"]
    assert ctypes.sizeof(EO._CDetEvalSpec) == 4 * 10 + 8 * (10 + 4 + 4) == 184
    assert [getattr(EO._CDetEvalSpec, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 36, 40, 120, 152]
    assert (EO.MAX_D, EO.MAX_M, EO.MAX_T, EO.MAX_A, EO.MAX_K, EO.MAX_R, EO.MAX_ROWS, EO.N_STATS) == (4096, 256, 10, 4, 65535, 1024, 1 << 20, 14)
    assert len(EO.STAT_NAMES) == 14 and EO.STAT_NAMES[12:] == ("ap_ref", "ar_ref")


def test_limits_match_the_header():
    import deteval_cases as DC
    lim = DC.limits()
    assert (lim["MAX_D"], lim["MAX_M"], lim["MAX_T"], lim["MAX_A"], lim["MAX_K"], lim["MAX_R"], lim["MAX_ROWS"]) == \
        (EO.MAX_D, EO.MAX_M, EO.MAX_T, EO.MAX_A, EO.MAX_K, EO.MAX_R, EO.MAX_ROWS)
    assert ctypes.sizeof(DC.CSpec) == ctypes.sizeof(EO._CDetEvalSpec)


BAD = [dict(K=0), dict(K=65536), dict(K=-1), dict(D=0), dict(D=4097), dict(M=-1), dict(M=257), dict(T=0), dict(T=11), dict(A=0), dict(A=5),
       dict(n_caps=0), dict(n_caps=4), dict(R=0), dict(R=1025), dict(max_dets={0: 0}), dict(max_dets={2: 101}), dict(max_dets={1: 200}),
       dict(max_dets={0: 11}), dict(max_dets={1: 0}),                             # not ascending
       dict(iou_thrs={3: NAN}), dict(area_lo={1: NAN}), dict(area_hi={3: NAN})]


@pytest.mark.parametrize("fn", sorted(CALLS))
def test_spec_checks(lib, fn):
    for bad in BAD:                                        # (a valid spec is never sent with the fake pointers)
        assert CALLS[fn](lib, _spec(**bad)) == INVALID, (fn, bad)
        assert fn.encode() + b":" in lib.gsr_last_error() and b"bad spec" in lib.gsr_last_error(), (fn, bad)
    assert CALLS[fn](lib, None) == INVALID and b"null spec" in lib.gsr_last_error()
    ok = _spec(iou_thrs={9: NAN}, T=9, area_hi={3: NAN}, A=3, max_dets={2: 0}, n_caps=2)      # beyond T, A and n_caps: not read
    assert _bytes(lib, ok) == 0


def test_row_limits(lib):
    cs = _spec()
    for B in (0, -1, (1 << 20) // 100 + 1):
        assert _match(lib, cs, B=B) == INVALID and b"B * D <= 2^20" in lib.gsr_last_error(), B
        assert _acc(lib, cs, N=B) == INVALID and b"N * D <= 2^20" in lib.gsr_last_error(), B
        assert _bytes(lib, cs, N=B) == INVALID and b"N * D <= 2^20" in lib.gsr_last_error(), B
    assert _acc(lib, cs, N=1 << 40) == INVALID
    assert _bytes(lib, _spec(D=4096, max_dets={2: 4096}), N=256) == 0 and _bytes(lib, _spec(D=4096), N=257) == INVALID


def test_null_and_misaligned_pointers(lib):
    cs = _spec()
    for n in MATCH_PTRS:
        assert _match(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
        if "ignore" not in n:                             # (bytes have no alignment)
            assert _match(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    for n in ACC_IN + ACC_OUT:
        assert _acc(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
    for n in ("dets", "dt_order", "dt_rank", "dt_match", "gt_cls", "npig"):
        assert _acc(lib, cs, **{n: FAKE + 2}) == INVALID and b"4-byte aligned" in lib.gsr_last_error(), n
    for n in ("rec_thrs", "precision", "scores", "recall"):
        assert _acc(lib, cs, **{n: FAKE + 4}) == INVALID and b"8-byte aligned" in lib.gsr_last_error(), n
    for n in ("precision", "recall", "stats"):
        assert _sum(lib, cs, **{n: None}) == INVALID and b"null" in lib.gsr_last_error(), n
        assert _sum(lib, cs, **{n: FAKE + 4}) == INVALID and b"8-byte aligned" in lib.gsr_last_error(), n
    assert _bytes(lib, cs, out=None) == INVALID and b"null bytes" in lib.gsr_last_error()
    # M == 0: the ground-truth pointers are not needed, the others still are
    m0 = _spec(M=0)
    assert _match(lib, m0, dets=None, gt_boxes=None, gt_cls=None, gt_ignore=None, gt_match=None) == INVALID and b"null dets" in lib.gsr_last_error()
    assert _acc(lib, m0, gt_cls=None, gt_ignore=None, npig=None) == INVALID and b"npig" in lib.gsr_last_error()


def test_workspace_checks(lib):
    cs = _spec()
    n = ctypes.c_int64(-1)
    assert lib.gsr_deteval_workspace_bytes(_ref(cs), 400, ctypes.byref(n)) == 0
    need = n.value
    assert need >= 5 * 4 * 400 * 100 and need % 256 == 0
    assert _acc(lib, cs, N=400, ws=None) == INVALID and b"null workspace" in lib.gsr_last_error()
    assert _acc(lib, cs, N=400, ws_bytes=need - 1) == INVALID and b"gsr_deteval_workspace_bytes" in lib.gsr_last_error()
    assert _acc(lib, cs, N=400, ws=FAKE + 8, ws_bytes=need) == INVALID and b"16-byte aligned" in lib.gsr_last_error()
    lib.gsr_deteval_workspace_bytes(_ref(cs), 2, ctypes.byref(n))
    assert n.value < need                                  # it grows with N


def test_cpu_tensors_raise_and_python_checks():
    dets, counts = torch.zeros(2, 100, 6), torch.zeros(2, 2, dtype=torch.int32)
    gb, gc = torch.zeros(2, 5, 4), torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        EO.match(dets, counts, gb, gc, COCO)
    m = EO.MatchOut(torch.zeros(2, 100, dtype=torch.int32), torch.zeros(2, 100, dtype=torch.int32), torch.zeros(2, 4, 10, 100, dtype=torch.int32),
                    torch.zeros(2, 4, 10, 100, dtype=torch.uint8), torch.zeros(2, 4, 5, dtype=torch.uint8), torch.zeros(2, 4, 10, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        EO.accumulate(dets, m, gc, torch.zeros(101, dtype=torch.float64), COCO)
    with pytest.raises(RuntimeError, match="no CPU path"):
        EO.summarize(torch.zeros(10, 101, 80, 4, 3, dtype=torch.float64), torch.zeros(10, 80, 4, 3, dtype=torch.float64), COCO)
    with pytest.raises(ValueError):
        EO.c_spec(COCO._replace(iou_thrs=(0.5,) * 11), 100, 5)
    with pytest.raises(ValueError):
        EO.c_spec(COCO._replace(max_dets=(1, 2, 3, 4)), 100, 5)
    with pytest.raises(TypeError):
        EO.match(dets.numpy(), counts, gb, gc, COCO)

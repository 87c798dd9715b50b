"""Named (reference, query) clouds and the two oracles for gsr_knn_query / gsr_knn_gather_mean (csrc/gsr_knnq.h,
csrc/gsr_knnq.hip.h), shared by tests/test_knnq_host_cpu.py (the scalar source built for the host) and
tests/test_gpu_knnq.py (the kernels).  Not a test module.  The clouds are the generators of tests/knn_cases.py.

Oracle E (exact): numpy float64 brute force with the contract's expression, d2 = (dx*dx + dy*dy) + dz*dz from float64
differences of the float32 coordinates, and a lexicographic (d2, index) order; NaN and +inf distances are no neighbours;
missing slots are -1 / +inf.  Indices and the float32 bits of d2 must be EQUAL: there is no tolerance.

Oracle M (mean): the float64 mean of the gathered rows.  The bound per element is 2 * 2^-24 * sum_j |v_j|: k - 1 additions
and one division, each within 2^-24 of the running magnitude (at most sum |v_j|), doubled.  An exact zero must be 0.
"""
import ctypes
import functools

import numpy as np

import host_build
import knn_cases as KC

FIN_SHELL, FIN_WHOLE, FIN_FALLBACK = KC.FIN_SHELL, KC.FIN_WHOLE, KC.FIN_FALLBACK
FIN_NONFINITE, FIN_OUTSIDE = 0x400, 0x800                       # KNNQ_FIN_* of csrc/gsr_knnq.h
EXCLUDE = 1                                                     # KNNQ_EXCLUDE_SAME_INDEX
MAX_K = 8
MEAN_BOUND = 2.0 * 2.0 ** -24


def _rng(name):
    return np.random.default_rng(sum(map(ord, "knnq-" + name)))


def _queries_in_box(name, n):
    """n float32 queries drawn uniformly in the bounding box of the named cloud's finite points"""
    p = KC.points(name)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    return (lo + _rng(name).random((n, 3)) * (hi - lo)).astype(np.float32)


def _pair_same(name):          # queries = references (no exclusion unless the case asks for it)
    return lambda: (KC.points(name), KC.points(name))


def _pair_box(name, n):
    return lambda: (KC.points(name), _queries_in_box(name, n))


def _slabs_middle():           # the 8 points in the empty middle as queries, the two slabs as references
    p = KC.points("slabs")
    return p[8:], p[:8]


def _outside():                # every query outside the references' box: beside a face, beyond a corner, and far away
    ref = KC.points("uniform")
    r = _rng("outside")
    q = r.random((90, 3))
    q[:30, 0] += 1.05                                   # just beside the +x face
    q[30:60] = 1.2 + 0.5 * r.random((30, 3))            # beyond the +++ corner
    q[60:] = -40.0 - 10.0 * r.random((30, 3))           # far away
    return ref, q.astype(np.float32)


def _poison_query(v):
    def make():
        ref = KC.points("uniform")
        q = _queries_in_box("uniform", 70)
        q[13, 1] = v
        q[40, :] = v
        return ref, q
    return make


def _tiny(R, Q):
    return lambda: (_rng(f"tiny{R}").random((R, 3)).astype(np.float32), _rng(f"tinyq{Q}").random((Q, 3)).astype(np.float32))


# name -> (make() -> (ref, qry), k, flags)
CASES = {
    # one-cell grids
    "p2": (_pair_same("p2"), 3, 0), "p3": (_pair_same("p3"), 3, EXCLUDE), "coincident": (_pair_box("coincident", 65), 5, 0),
    # zero distances: the index rule decides
    "twopos": (_pair_same("twopos"), 5, 0), "twopos-self": (_pair_same("twopos"), 8, EXCLUDE),
    "duplicates": (_pair_same("duplicates"), 4, EXCLUDE),
    # ties everywhere, points on cell faces
    "lattice": (_pair_same("lattice"), 8, 0), "lattice-self": (_pair_same("lattice"), 5, EXCLUDE),
    "lattice-faces": (_pair_same("lattice-faces"), 7, EXCLUDE),
    "line": (_pair_box("line", 257), 5, 0),
    "flat": (_pair_box("flat", 257), 6, 0),
    "clusters": (_pair_box("clusters", 257), 5, 0),
    "slabs": (_slabs_middle, 5, 0),
    "outliers": (_pair_same("outliers"), 3, EXCLUDE),
    "uniform-off1e5": (_pair_same("uniform-off1e5"), 5, EXCLUDE),
    "uniform-self3": (_pair_same("uniform"), 3, EXCLUDE),
    "uniform-same": (_pair_same("uniform"), 3, 0),
    "outside": (_outside, 5, 0),
    "nan-point": (_pair_box("nan-point", 63), 5, 0), "inf-point": (_pair_box("inf-point", 63), 5, 0),
    "nan-point-self": (_pair_same("nan-point"), 2, EXCLUDE), "inf-point-self": (_pair_same("inf-point"), 2, EXCLUDE),
    "nan-query": (_poison_query(np.nan), 5, 0), "inf-query": (_poison_query(np.inf), 5, 0),
}
# R in {0, 1, 2, k-1, k, k+1} at k = 5, Q in {0, 1, 63, 64, 65, 257}, and every k
for _R, _Q in ((0, 1), (0, 65), (1, 64), (2, 63), (4, 65), (5, 257), (6, 64), (6, 0), (0, 0)):
    CASES[f"r{_R}-q{_Q}"] = (_tiny(_R, _Q), 5, 0)
for _k in range(1, MAX_K + 1):
    CASES[f"uniform-k{_k}"] = (_pair_box("uniform", 65), _k, 0)
    CASES[f"self7-k{_k}"] = (_pair_same("p7"), _k, EXCLUDE)
NAMES = list(CASES)

# what the path test holds the named cases to (host build's finish codes)
# ('coincident' is one OCCUPIED cell, not a one-cell grid: knn_make_grid gives coinciding points extents of 1e-6 and 7 cells
# per axis, all references in cell 0 and every query in it too)
ONE_CELL = ("p2", "p3", "inf-point", "inf-point-self", "r1-q64")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> ref [R,3] float32, qry [Q,3] float32 (read-only, the same arrays every time), k, flags"""
    make, k, flags = CASES[name]
    ref, qry = make()
    ref, qry = KC._f32(ref), KC._f32(qry)
    if ref is qry or np.shares_memory(ref, qry):
        qry = ref
    for a in (ref, qry):
        a.setflags(write=False)
    return ref, qry, k, flags


# ---- oracle E -------------------------------------------------------------------------------------------------------------
def oracle_e(ref, qry, k, flags=0, rows=None):
    """-> idx [n,k] int32, d2 [n,k] float32 for the given query rows (all when None)"""
    ref64, qry64 = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(qry, np.float64).reshape(-1, 3)
    rows = np.arange(len(qry64)) if rows is None else np.asarray(rows, np.int64)
    R = len(ref64)
    idx = np.full((len(rows), k), -1, np.int32)
    d2o = np.full((len(rows), k), np.inf, np.float32)
    if R == 0 or len(rows) == 0:
        return idx, d2o
    chunk = max(1, (2 << 20) // R)
    ar = np.arange(R)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(rows), chunk):
            rr = rows[s:s + chunk]
            q = qry64[rr]
            dx = ref64[None, :, 0] - q[:, None, 0]
            dy = ref64[None, :, 1] - q[:, None, 1]
            dz = ref64[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            d2[~np.isfinite(d2)] = np.inf
            if flags & EXCLUDE:
                d2[np.arange(len(rr)), rr] = np.inf
            kk = min(k, R) - 1
            thr = np.partition(d2, kk, axis=1)[:, kk]               # the k-th smallest value: only rows up to it can be taken
            for i in range(len(rr)):
                cand = ar[d2[i] <= thr[i]]                          # ascending index
                order = cand[np.lexsort((cand, d2[i][cand]))][:k]   # d2 first, then the index
                order = order[np.isfinite(d2[i][order])]
                idx[s + i, :len(order)] = order
                d2o[s + i, :len(order)] = d2[i][order].astype(np.float32)
    return idx, d2o


@functools.lru_cache(maxsize=None)
def oracle(name):
    ref, qry, k, flags = case(name)
    idx, d2 = oracle_e(ref, qry, k, flags)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def check_exact(tag, name, got_idx, got_d2, want=None):
    """indices equal and d2 equal bit for bit"""
    want_idx, want_d2 = oracle(name) if want is None else want
    got_idx, got_d2 = np.asarray(got_idx), np.asarray(got_d2)
    assert got_idx.dtype == np.int32 and got_d2.dtype == np.float32, (tag, name, got_idx.dtype, got_d2.dtype)
    assert got_idx.shape == want_idx.shape and got_d2.shape == want_d2.shape, (tag, name, got_idx.shape, want_idx.shape)
    bad = np.nonzero((got_idx != want_idx).any(axis=1))[0] if got_idx.size else np.zeros(0, np.int64)
    print(f"knnq {tag} {name}: Q {got_idx.shape[0]} k {got_idx.shape[1]} rows with a wrong index {len(bad)}")
    assert len(bad) == 0, (tag, name, bad[:5], got_idx[bad[:5]], want_idx[bad[:5]])
    assert np.array_equal(got_d2.view(np.uint32), want_d2.view(np.uint32)), (tag, name, "d2 bits differ")


# ---- oracle M -------------------------------------------------------------------------------------------------------------
def oracle_m(idx, src):
    """-> mean [Q,cols] float64, bound [Q,cols] float64 for src [R,cols]; an index outside 0..R-1 is missing"""
    idx = np.asarray(idx, np.int64)
    src = np.asarray(src, np.float64)
    R = src.shape[0]
    ok = (idx >= 0) & (idx < R)
    rows = src[np.clip(idx, 0, max(R - 1, 0))] if R else np.zeros(idx.shape + src.shape[1:])
    rows = np.where(ok[:, :, None], rows, 0.0)
    m = ok.sum(axis=1)
    mean = rows.sum(axis=1) / np.maximum(m, 1)[:, None]
    return mean, MEAN_BOUND * np.abs(rows).sum(axis=1)


def check_mean(tag, got, idx, src):
    mean, bound = oracle_m(idx, src)
    got = np.asarray(got, np.float64).reshape(mean.shape)
    err = np.abs(got - mean)
    zero = bound == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()))), (tag, "an exact zero must be 0")
    worst = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f"knnq mean {tag}: {got.shape} worst error / bound {worst:.3f}")
    assert worst <= 1.0, (tag, worst)


# ---- the host build -------------------------------------------------------------------------------------------------------
def host_lib():
    lib = host_build.host_lib("knnq")
    lib.kq_query.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32,
                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.kq_query.restype = ctypes.c_int
    lib.kq_gather_mean.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                   ctypes.c_int32, ctypes.c_void_p]
    lib.kq_gather_mean.restype = ctypes.c_int
    return lib


def host_query(lib, ref, qry, k, flags=0):
    """-> idx [Q,k] int32, d2 [Q,k] float32, finish [Q] int32, dims; outputs start as -7 / NaN / -1 so that a query the
    build never wrote shows"""
    ref, qry = KC._f32(ref), KC._f32(qry)
    R, Q = len(ref), len(qry)
    idx = np.full((Q, k), -7, np.int32)
    d2 = np.full((Q, k), np.nan, np.float32)
    fin = np.full(Q, -1, np.int32)
    dims = np.zeros(3, np.int32)
    rc = lib.kq_query(ref.ctypes.data if R else None, R, qry.ctypes.data if Q else None, Q, k, flags,
                      idx.ctypes.data if Q else None, d2.ctypes.data if Q else None, fin.ctypes.data if Q else None,
                      dims.ctypes.data)
    assert rc == 0, rc
    return idx, d2, fin, tuple(int(d) for d in dims)


@functools.lru_cache(maxsize=None)
def host_result(name):
    ref, qry, k, flags = case(name)
    return host_query(host_lib(), ref, qry, k, flags)


def host_gather_mean(lib, idx, src):
    idx = np.ascontiguousarray(idx, np.int32)
    R = src.shape[0]
    src = np.ascontiguousarray(src, np.float32).reshape(R, -1) if R else np.zeros((0, int(np.prod(src.shape[1:]))), np.float32)
    Q, k = idx.shape
    cols = src.shape[1]
    dst = np.full((Q, cols), np.nan, np.float32)
    rc = lib.kq_gather_mean(idx.ctypes.data if Q else None, Q, k, R, src.ctypes.data if R else None, cols,
                            dst.ctypes.data if Q else None)
    assert rc == 0, rc
    return dst


def mean_inputs(R=300, Q=130, k=5, seed=0):
    """idx [Q,k] with missing slots, whole missing rows and out-of-range indices, and the seven attribute tensors' shapes"""
    r = np.random.default_rng(900 + seed)
    idx = r.integers(0, R, (Q, k)).astype(np.int32)
    idx[3, 2:] = -1                                      # (nothing at k <= 2)
    idx[7, :] = -1                                       # a row of -1: zeros
    idx[11, 1 % k] = R                                   # not an index: skipped
    idx[12, 0] = R + 1000
    idx[13, 4 % k] = -5
    shapes = dict(xyz=(3,), f_dc=(1, 3), f_rest=(15, 3), scaling=(3,), rotation=(4,), opacity=(1,), objects=(1, 16))
    tensors = {n: (r.standard_normal((R,) + s) * 10.0 ** r.integers(-2, 3)).astype(np.float32) for n, s in shapes.items()}
    tensors["opacity"][:40] = 0.0                        # exact zeros
    return idx, tensors

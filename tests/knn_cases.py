"""Named point clouds, the float64 oracle and the tolerance for gsr_knn_dist2 (csrc/gsr_knn.h, csrc/gsr_knn.hip.h), shared by
tests/test_knn_host_cpu.py (the scalar source built for the host) and tests/test_gpu_knn.py (the kernels).

Oracle: float64 brute force in row chunks, from coordinate DIFFERENCES (not the |a|^2 + |b|^2 - 2ab expansion, which
cancels at large offsets): the squared distance to every other point, the three smallest, their mean.  Squared distances that
are NaN or +inf are not neighbours, and with fewer than three neighbours the missing ones are FLT_MAX with the sum and the
division in float32 -- the contract written into csrc/gsr_knn.h.

Tolerance: relative 16 * 2^-24, no absolute term; an exact zero must be exactly 0, +inf must be +inf.  Inputs are exact
floats; one rounding per difference (its square carries two), the square, two additions, the three-term sum and the division
make at most 8 units of 2^-24, doubled.  Taking another neighbour among near-ties moves the value by rounding only.
"""
import ctypes
import functools
import os

import numpy as np
import torch

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
HM = os.path.join(ROOT, "tests", "host_math")
SRC = os.path.join(HM, "knn_host.cpp")

FLT_MAX = np.float32(np.finfo(np.float32).max)
RTOL = 16.0 * 2.0 ** -24
MAX_SHELL = 10
FIN_SHELL, FIN_WHOLE, FIN_FALLBACK = 0xff, 0x100, 0x200      # KNN_FIN_* of csrc/gsr_knn.h


# ---- the clouds ------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(sum(map(ord, name)))          # str hashes change per process


def _tg(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))  # the seeds tests/test_gpu_knn.py has always used


def _uniform():
    return _rng("uniform").random((6000, 3), dtype=np.float32)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))


def _small(n):
    return lambda: _rng(f"p{n}").random((n, 3), dtype=np.float32)


# One cell needs every extent <= cbrt(3 vol / P): any single point; two points whose difference is nearly a cube's diagonal;
# three points only when the bounding box is a cube (extent 1 here, so that cbrt gives exactly 1).
def _p2():
    return np.array([[0.1, 0.2, 0.3], [0.6, 0.75, 0.8]], np.float32)


def _p3():
    return np.array([[2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [2.25, 2.5, 2.75]], np.float32)


def _coincident():
    return np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (700, 1))


def _twopos():   # 255 + 2: the pair has one coincident neighbour (0) and two at the full extent
    a, b = np.array([0.25, 0.5, -1.0], np.float32), np.array([3.25, 2.5, 1.0], np.float32)
    return np.concatenate([np.tile(a, (255, 1)), np.tile(b, (2, 1))])


def _duplicates():
    base = torch.rand(500, 3, generator=_tg("duplicates"))
    return torch.cat([base, base[:200], base[:50]]).numpy()


def _line():     # y and z extents 1e-3 of x: 6000 points ask for ~1260 cells along x, the cap gives 256 x 2 x 2
    return _rng("line").random((6000, 3), dtype=np.float32) * np.array([1.0, 1e-3, 1e-3], np.float32)


def _flat():     # a degenerate bounding box (all z equal)
    pts = torch.rand(3000, 3, generator=_tg("flat"))
    pts[:, 2] = 0.25
    return pts.numpy()


def _lattice():  # 12 steps per axis, 6000 points on 1728 positions: ties everywhere
    return _rng("lattice").integers(0, 12, (6000, 3)).astype(np.float32) * np.float32(0.25)


def _lattice_faces(m=10):   # m + 1 steps, P = 3 m^3: extent m, cell exactly 1, so the points sit exactly on cell faces
    ijk = _rng("lattice-faces").integers(0, m + 1, (3 * m ** 3, 3))
    ijk[0], ijk[1] = 0, m
    return ijk.astype(np.float32)


def _clusters():  # 400 clusters of 20, spread 1e-5 of the extent: many points per cell, cell faces cut clusters
    r = _rng("clusters")
    c = r.random((400, 1, 3))
    return (c + 1e-5 * r.standard_normal((400, 20, 3))).reshape(-1, 3)


SLABS_SEED = 1


def _slabs(seed=None):   # two dense slabs and 8 points in the empty middle, which need more than MAX_SHELL shells
    r = np.random.default_rng(SLABS_SEED if seed is None else seed)
    p = r.random((40000, 3))
    p[:, 0] *= 0.05
    p[20000:, 0] += 0.95
    p[:8, 0] = 0.5 + 0.001 * np.arange(8)
    return p


def _outliers():  # isolated points far from a dense cluster
    g = _tg("outliers")
    return torch.cat([torch.randn(4000, 3, generator=g) * 0.1, torch.randn(12, 3, generator=g) * 500]).numpy()


NAN_AT, INF_AT = (777, 1), (1234, 0)


def _poisoned(name, at, v):
    def make():
        p = _rng(name).random((2000, 3), dtype=np.float32)
        p[at] = v
        return p
    return make


CASES = {
    "p1": _small(1), "p2": _p2, "p3": _p3, "p4": _small(4), "p5": _small(5), "p7": _small(7),
    "coincident": _coincident,
    "twopos": _twopos,
    "duplicates": _duplicates,
    "uniform": _uniform,
    "uniform-ext1e-3": lambda: _uniform() * np.float32(1e-3),
    "uniform-ext1e6": lambda: _uniform() * np.float32(1e6),
    "uniform-off1000": lambda: _uniform() + np.float32(1000.0),
    "uniform-off1e5": lambda: _uniform() + np.float32(1e5),
    "line": _line,
    "flat": _flat,
    "lattice": _lattice,
    "lattice-faces": _lattice_faces,
    "clusters": _clusters,
    "slabs": _slabs,
    "outliers": _outliers,
    "nan-point": _poisoned("nan-point", NAN_AT, np.nan),
    "inf-point": _poisoned("inf-point", INF_AT, np.inf),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def _points(name):
    p = _f32(CASES[name]())
    p.setflags(write=False)
    return p


def points(name) -> np.ndarray:
    """[P,3] float32, read-only, the same array every time"""
    return _points(name)


# ---- what the coverage test holds every case to (from the host build's finish codes and dims) ------------------------------
# dims: the grid; fallback: points that took the full sweep (exact count, or ">=k"); whole: True when SOME point stopped
# because its block covered the grid; shell: the largest shell index seen
COVERAGE = {
    "p1": dict(dims=(1, 1, 1), fallback=0, whole=True, shell=0),
    "p2": dict(dims=(1, 1, 1), fallback=0, whole=True, shell=0),
    "p3": dict(dims=(1, 1, 1), fallback=0, whole=True, shell=0),
    "inf-point": dict(dims=(1, 1, 1), fallback=0, whole=True, shell=0),
    "line": dict(dims=(256, 2, 2), fallback=0),
    "slabs": dict(dims=(24, 24, 24), fallback=">=3", shell=10),
    "outliers": dict(fallback=0),
}
ONE_CELL = ("p1", "p2", "p3", "inf-point")


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def oracle_rows(pts: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """float64 [len(rows)]: the contract's value for the given rows of pts (not rounded to float32, except where the contract
    itself is float32 arithmetic)"""
    x = torch.from_numpy(np.array(pts, np.float64))
    P = x.shape[0]
    rows_t = torch.from_numpy(np.array(rows, np.int64))
    k = min(3, P)
    best = torch.full((len(rows_t), 3), float("inf"), dtype=torch.float64)
    chunk = max(1, (4 << 20) // max(P, 1))
    for s in range(0, len(rows_t), chunk):
        r = rows_t[s:s + chunk]
        d2 = torch.zeros(len(r), P, dtype=torch.float64)
        for a in range(3):
            d2 += (x[r, a][:, None] - x[None, :, a]).square_()
        d2[torch.arange(len(r)), r] = float("inf")
        d2[~torch.isfinite(d2)] = float("inf")              # NaN and +inf distances are not neighbours
        if k:
            best[s:s + chunk, :k] = torch.topk(d2, k, dim=1, largest=False).values
    b = best.numpy()
    full = np.isfinite(b).all(axis=1)
    out = np.empty(len(rows_t), np.float64)
    out[full] = b[full].sum(axis=1) / 3.0
    # fewer than three neighbours: FLT_MAX for the missing ones, the sum and the division in float32 as the kernel does them
    with np.errstate(over="ignore"):
        for i in np.nonzero(~full)[0]:
            d = [np.float32(v) if np.isfinite(v) else FLT_MAX for v in b[i]]
            out[i] = np.float32(np.float32(np.float32(d[0] + d[1]) + d[2]) / np.float32(3.0))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    pts = points(name)
    rows = sample_rows(name)
    ref = oracle_rows(pts, rows)
    ref.setflags(write=False)
    return ref


def oracle(name) -> np.ndarray:
    """the oracle on sample_rows(name), computed once"""
    return _oracle(name)


@functools.lru_cache(maxsize=None)
def _sample_rows(name):
    P = points(name).shape[0]
    if name != "slabs":
        rows = np.arange(P)
    else:   # a sample: the 8 middle points (every point the host build sends to the fallback is one of them; the host test
        # asserts that), their neighbourhood in index order, and 3000 drawn rows
        rows = np.unique(np.concatenate([np.arange(64), _rng("slabs-sample").choice(P, 3000, replace=False)]))
    rows.setflags(write=False)
    return rows


def sample_rows(name) -> np.ndarray:
    return _sample_rows(name)


def worst_ratio(got: np.ndarray, ref: np.ndarray) -> float:
    """max over the points of |got - ref| / (RTOL * ref); exact zeros and infinities must match exactly (inf otherwise)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    exact = (ref == 0) | ~np.isfinite(ref)
    if not np.array_equal(got[exact], ref[exact]):
        return float("inf")
    if exact.all():
        return 0.0
    if not np.isfinite(got[~exact]).all():
        return float("inf")
    return float((np.abs(got[~exact] - ref[~exact]) / (RTOL * ref[~exact])).max())


def check(tag, name, got, ref):
    """print the worst error-to-bound ratio, then hold it to 1"""
    w = worst_ratio(got, ref)
    print(f"knn {tag} {name}: P {points(name).shape[0]} worst error / bound {w:.3f}")
    assert w <= 1.0, (tag, name, w)
    return w


# ---- the host build -----------------------------------------------------------------------------------------------------------
def host_lib():
    lib = host_build.host_lib("knn")
    lib.kh_dist2.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.kh_dist2.restype = ctypes.c_int
    return lib


def host_dist2(lib, pts: np.ndarray):
    """-> out [P] float32, finish [P] int32, dims (dx, dy, dz); out and finish start as NaN / -1, so a point the build
    never wrote shows"""
    pts = _f32(pts)
    P = pts.shape[0]
    out = np.full(P, np.nan, np.float32)
    fin = np.full(P, -1, np.int32)
    dims = np.zeros(3, np.int32)
    assert lib.kh_dist2(pts.ctypes.data, P, out.ctypes.data, fin.ctypes.data, dims.ctypes.data) == 0
    return out, fin, tuple(int(d) for d in dims)


@functools.lru_cache(maxsize=None)
def host_result(name):
    return host_dist2(host_lib(), points(name))


def fnv1a(out: np.ndarray) -> int:
    """the hash the stand-alone program prints over a result's bytes"""
    h = 2166136261
    for b in np.ascontiguousarray(out, np.float32).tobytes():
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


# ---- fuzz -------------------------------------------------------------------------------------------------------------------
FUZZ_KINDS = ("uniform", "gauss", "clusters", "outliers")


def fuzz_cloud(seed: int):
    """-> kind, [P,3] float32: P in 4..8000 (log-uniform), extent 1e-3..1e6 and, for half of them, an offset of 0.1..1e5 extents"""
    r = np.random.default_rng(10_000 + seed)
    kind = FUZZ_KINDS[seed % len(FUZZ_KINDS)]
    P = int(np.exp(r.uniform(np.log(4), np.log(8000))))
    if kind == "uniform":
        p = r.random((P, 3))
    elif kind == "gauss":
        p = r.standard_normal((P, 3)) * r.uniform(0.05, 1.0, 3)
    elif kind == "clusters":
        nc = max(1, P // 20)
        p = r.random((nc, 3))[r.integers(0, nc, P)] + 10.0 ** r.uniform(-6, -3) * r.standard_normal((P, 3))
    else:
        p = r.standard_normal((P, 3)) * 0.1
        far = r.integers(0, P, max(1, P // 300))
        p[far] = r.standard_normal((len(far), 3)) * 500
    ext = 10.0 ** r.uniform(-3, 6)
    off = ext * 10.0 ** r.uniform(-1, 5) * r.choice([-1.0, 1.0], 3) * (r.random() < 0.5)
    return kind, _f32(p * ext + off)

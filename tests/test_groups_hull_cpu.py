"""The groups set-up's convex hull (csrc/gsr_hull.h) on the host, through a g++ build of the header
(tests/host_math/hull_harness.cpp): closed-form hulls, degenerate inputs, the self-check on random clouds, a sanitizer
build, and agreement with the reference's construction (scipy Delaunay find_simplex).  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_math", "hull_harness.cpp")
OK, DEGENERATE = 0, 1


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hull") / "libhull.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-I", CSRC, SRC,
                    "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.hh_convex_hull.restype = ctypes.c_int
    lib.hh_convex_hull.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                   ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_void_p]
    return lib


def hull(lib, pts):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    cap = max(16, 2 * pts.shape[0])
    planes = np.zeros((cap, 4))
    nf = ctypes.c_int64(0)
    bbox = np.zeros(6)
    info = np.zeros(3)
    st = lib.hh_convex_hull(pts.ctypes.data, pts.shape[0], planes.ctypes.data, cap, ctypes.byref(nf), bbox.ctypes.data,
                            info.ctypes.data)
    return st, planes[:nf.value].copy(), bbox, dict(D=info[0], tau=info[1], worst=info[2])


def dist(planes, q):
    """The library's evaluation order, every operation rounded on its own: ((nx*x + ny*y) + nz*z) - c."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    s = planes[None, :, 0] * q[:, 0:1]
    s = s + planes[None, :, 1] * q[:, 1:2]
    s = s + planes[None, :, 2] * q[:, 2:3]
    return s - planes[None, :, 3]


def inside(planes, bbox, tau, q):
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    inbox = np.all((q >= bbox[:3] - tau) & (q <= bbox[3:] + tau), axis=1)
    return inbox & np.all(dist(planes, q) <= tau, axis=1) if len(planes) else np.zeros(len(q), bool)


def cube_corners(lo=0.0, hi=1.0):
    return np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float64)


def face_set(planes, decimals=12):
    return sorted({(tuple(np.round(p[:3], decimals) + 0.0), round(float(p[3]), decimals) + 0.0) for p in planes})


def test_unit_cube(hh):
    st, planes, bbox, info = hull(hh, cube_corners())
    assert st == OK and len(planes) == 12                       # two triangles per face, coplanar facets not merged
    assert np.allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0, atol=1e-15)
    want = [((-1.0, 0.0, 0.0), 0.0), ((0.0, -1.0, 0.0), 0.0), ((0.0, 0.0, -1.0), 0.0),
            ((0.0, 0.0, 1.0), 1.0), ((0.0, 1.0, 0.0), 1.0), ((1.0, 0.0, 0.0), 1.0)]
    assert face_set(planes) == sorted(want)
    assert np.allclose(bbox, [0, 0, 0, 1, 1, 1]) and info["tau"] == pytest.approx(1e-9 * np.sqrt(3.0))
    # query points 1e-4 inside and outside the middle of every face
    for axis in range(3):
        for side, sign in ((0.0, 1.0), (1.0, -1.0)):
            q_in = np.full(3, 0.5); q_in[axis] = side + sign * 1e-4
            q_out = np.full(3, 0.5); q_out[axis] = side - sign * 1e-4
            assert inside(planes, bbox, info["tau"], q_in)[0] and not inside(planes, bbox, info["tau"], q_out)[0]


def test_tetrahedron(hh):
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    st, planes, bbox, info = hull(hh, pts)
    assert st == OK and len(planes) == 4
    s = 1.0 / np.sqrt(3.0)
    want = [((-1.0, 0.0, 0.0), 0.0), ((0.0, -1.0, 0.0), 0.0), ((0.0, 0.0, -1.0), 0.0), ((s, s, s), s)]
    assert face_set(planes) == face_set(np.array([[*n, c] for n, c in want]))
    tau = info["tau"]
    c = np.array([0.25, 0.25, 0.25])
    assert inside(planes, bbox, tau, c)[0]
    n = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    on = np.array([1 / 3, 1 / 3, 1 / 3])                       # centre of the slanted face
    assert inside(planes, bbox, tau, on - 1e-4 * n)[0] and not inside(planes, bbox, tau, on + 1e-4 * n)[0]


def test_cube_with_interior_points(hh):
    rng = np.random.default_rng(3)
    pts = np.concatenate([cube_corners(-2.0, 3.0), rng.uniform(-1.9, 2.9, size=(5000, 3))])
    rng.shuffle(pts)
    st, planes, bbox, info = hull(hh, pts)
    assert st == OK and len(planes) == 12
    assert face_set(planes) == sorted([((-1.0, 0.0, 0.0), 2.0), ((0.0, -1.0, 0.0), 2.0), ((0.0, 0.0, -1.0), 2.0),
                                       ((0.0, 0.0, 1.0), 3.0), ((0.0, 1.0, 0.0), 3.0), ((1.0, 0.0, 0.0), 3.0)])
    assert info["worst"] <= info["tau"]


@pytest.mark.parametrize("case", ["coplanar", "three", "identical", "collinear"])
def test_degenerate(hh, case):
    rng = np.random.default_rng(5)
    if case == "coplanar":
        uv = rng.uniform(-1, 1, size=(200, 2))
        pts = np.stack([uv[:, 0], uv[:, 1], 0.5 * uv[:, 0] - 0.25 * uv[:, 1] + 2.0], axis=1)   # a tilted plane
    elif case == "three":
        pts = rng.normal(size=(3, 3))
    elif case == "identical":
        pts = np.tile([[1.5, -2.0, 0.25]], (100, 1))
    else:
        t = rng.uniform(-1, 1, size=100)
        pts = np.stack([t, 2 * t + 1, -t], axis=1)
    st, planes, _, _ = hull(hh, pts)
    assert st == DEGENERATE and len(planes) == 0


@pytest.mark.parametrize("M", [10, 100, 1000, 20000, 200000])
@pytest.mark.parametrize("kind", ["gauss", "ball", "box_surface"])
def test_self_check_holds(hh, M, kind):
    rng = np.random.default_rng(M + len(kind))
    if kind == "gauss":
        pts = rng.normal(size=(M, 3)) * [3.0, 1.0, 0.2] + [10.0, -4.0, 7.0]
    elif kind == "ball":
        v = rng.normal(size=(M, 3))
        pts = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, size=(M, 1)) ** (1 / 3)
    else:
        pts = rng.uniform(-1, 1, size=(M, 3)) * [2.0, 3.0, 5.0]
        ax = rng.integers(0, 3, size=M)
        pts[np.arange(M), ax] = np.sign(pts[np.arange(M), ax]) * np.array([2.0, 3.0, 5.0])[ax]
        pts = pts.astype(np.float32).astype(np.float64)           # float32 positions, as the scenes hold them
        pts[1::5] = pts[0::5][: len(pts[1::5])]                     # duplicates
    st, planes, bbox, info = hull(hh, pts)
    assert st == OK, st
    assert len(planes) >= 4 and info["worst"] <= info["tau"]
    # the check the library made, repeated here on a sample
    idx = rng.choice(M, size=min(M, 5000), replace=False)
    assert np.all(dist(planes, pts[idx]) <= info["tau"])


def test_sanitized_build(tmp_path):
    exe = str(tmp_path / "hull_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-DHULL_MAIN", "-pthread", "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def _cloud(kind, rng, M):
    if kind == "blob":
        return rng.normal(size=(M, 3)) * [2.0, 0.7, 1.3] + [3.0, 1.0, 5.0]
    # box-surface cloud: points on the walls and roof of three boxes (the city scenes' structure)
    out = []
    for cx, cy, sx, sy, h in ((0.0, 0.0, 4.0, 3.0, 10.0), (5.0, 1.0, 2.0, 5.0, 6.0), (-3.0, 4.0, 3.0, 3.0, 14.0)):
        n = M // 3
        u, v = rng.uniform(-0.5, 0.5, n), rng.uniform(0, 1, n)
        f = rng.integers(0, 5, n)
        x = np.where(f < 2, cx + u * sx, np.where(f < 4, cx + np.where(f == 2, -0.5, 0.5) * sx, cx + u * sx))
        y = np.where(f < 2, cy + np.where(f == 0, -0.5, 0.5) * sy, np.where(f < 4, cy + u * sy, cy + (v - 0.5) * sy))
        z = np.where(f < 4, v * h, h)
        out.append(np.stack([x, y, z], axis=1))
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("kind", ["blob", "box_surface"])
def test_against_reference_delaunay(hh, kind):
    """The planes' verdict (numpy float64) against the reference's construction, Delaunay(filtered).find_simplex(q) >= 0
    (scratch/edit_object_removal.py:59-63), on 20 000 query points; only points within 1e-6 D of the boundary are left
    out."""
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(11 if kind == "blob" else 12)
    pts = _cloud(kind, rng, 6000)
    # the reference's IQR filter, float32 (edit_object_removal.py:52-56)
    Q1, Q3 = np.percentile(pts, 25, axis=0), np.percentile(pts, 75, axis=0)
    IQR = Q3 - Q1
    filt = pts[~np.any((pts < Q1 - IQR) | (pts > Q3 + IQR), axis=1)]
    st, planes, bbox, info = hull(hh, filt.astype(np.float64))
    assert st == OK
    lo, hi = filt.min(axis=0).astype(np.float64), filt.max(axis=0).astype(np.float64)
    span = hi - lo
    q = lo - 0.15 * span + rng.uniform(0, 1, size=(20000, 3)) * 1.3 * span
    mine = inside(planes, bbox, info["tau"], q)
    ref = spatial.Delaunay(filt).find_simplex(q) >= 0
    d = dist(planes, q).max(axis=1)
    near = np.abs(d) <= 1e-6 * info["D"]
    print(f"[hull vs Delaunay {kind}] {len(filt)} points, {len(planes)} facets, {int(near.sum())} of {len(q)} queries "
          f"within 1e-6 D of the boundary left out, {int(mine.sum())} inside")
    assert 1000 < int(mine.sum()) < 19000
    assert np.array_equal(mine[~near], ref[~near])

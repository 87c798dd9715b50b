"""gsr_knn_dist2's scalar source (csrc/gsr_knn.h) on the CPU: tests/host_math/knn_host.cpp runs the device pipeline's steps
in plain loops over the header the kernels compile.  Held to the float64 oracle of tests/knn_cases.py on every named case and
on a fuzz; the finish codes prove which path each case takes; a stand-alone build runs every case under the address and
undefined-behaviour sanitizers; and the CPU branch of simple_knn._C follows the header's contract below 4 points.  No GPU."""
import subprocess

import numpy as np
import pytest
import torch

import knn_cases as KC


@pytest.fixture(scope="module")
def lib():
    return KC.host_lib()


@pytest.mark.parametrize("name", KC.NAMES)
def test_host_build_matches_oracle(lib, name):
    out, fin, dims = KC.host_result(name)
    assert (fin >= 0).all(), "points the search never wrote"
    rows = KC.sample_rows(name)
    if name == "slabs":   # the oracle covers a sample: it must hold every point that took the full sweep
        assert set(np.nonzero(fin & KC.FIN_FALLBACK)[0]) <= set(rows.tolist())
    KC.check("host", name, out[rows], KC.oracle(name))


def test_poisoned_points():
    """a NaN or an infinite coordinate: +inf for that point, and the others are the oracle's values over the finite points"""
    for name, at in (("nan-point", KC.NAN_AT), ("inf-point", KC.INF_AT)):
        pts = KC.points(name)
        out, _, _ = KC.host_result(name)
        assert out[at[0]] == np.inf and KC.oracle(name)[at[0]] == np.inf
        keep = np.arange(len(pts)) != at[0]
        sub = KC.oracle_rows(pts[keep], np.arange(keep.sum()))
        assert np.isfinite(sub).all() and np.array_equal(sub, KC.oracle(name)[keep])
        KC.check("host finite subset", name, out[keep], sub)


def test_fewer_than_four_points():
    """the missing-neighbour contract in numbers: +inf for P <= 2, (d0 + d1 + FLT_MAX) / 3 in float32 for P = 3"""
    for name in ("p1", "p2"):
        assert np.isposinf(KC.host_result(name)[0]).all() and np.isposinf(KC.oracle(name)).all()
    out = KC.host_result("p3")[0]
    assert np.array_equal(out, np.full(3, KC.FLT_MAX / np.float32(3.0), np.float32))    # d0 + d1 is far below FLT_MAX's ulp
    assert np.array_equal(out.astype(np.float64), KC.oracle("p3"))


def test_cases_take_the_paths_they_claim():
    seen = dict(fallback=[], one_cell=[], cap=[], whole=[])
    for name in KC.NAMES:
        out, fin, dims = KC.host_result(name)
        nfb = int(((fin & KC.FIN_FALLBACK) != 0).sum())
        nwhole = int(((fin & KC.FIN_WHOLE) != 0).sum())
        shell = int((fin & KC.FIN_SHELL).max())
        print(f"knn paths {name}: P {len(out)} dims {dims} fallback {nfb} whole-grid {nwhole} largest shell {shell}")
        assert shell <= KC.MAX_SHELL and not ((fin & KC.FIN_FALLBACK != 0) & (fin & KC.FIN_WHOLE != 0)).any()
        want = KC.COVERAGE.get(name, {})
        if "dims" in want:
            assert dims == want["dims"], (name, dims)
        if "fallback" in want:
            assert (nfb >= int(want["fallback"][2:])) if isinstance(want["fallback"], str) else (nfb == want["fallback"]), (name, nfb)
        if "whole" in want:
            assert (nwhole > 0) == want["whole"], (name, nwhole)
        if "shell" in want:
            assert shell == want["shell"], (name, shell)
        if nfb:
            seen["fallback"].append(name)
        if dims == (1, 1, 1):
            seen["one_cell"].append(name)
            assert nwhole == len(out)                       # one cell: every point stops at shell 0, nothing left to scan
        if max(dims) == 256:
            seen["cap"].append(name)
        if nwhole:
            seen["whole"].append(name)
    assert seen["fallback"] == ["slabs"]                    # 'outliers' is NOT a test of the fallback
    assert tuple(seen["one_cell"]) == KC.ONE_CELL
    assert seen["cap"] == ["line", "flat"]                 # flat: all z equal, so x and y ask for more than 256 cells
    assert {"p4", "p5", "p7", "twopos"} <= set(seen["whole"])
    for name in ("p4", "p5", "p7"):                         # the smallest grids of more than one cell
        assert 1 < int(np.prod(KC.host_result(name)[2])) <= 8
    # in 'slabs' the fallback points are among the 8 placed in the empty middle
    fin = KC.host_result("slabs")[1]
    assert np.nonzero(fin & KC.FIN_FALLBACK)[0].max() < 8


def test_fuzz_against_oracle(lib):
    worst = {k: 0.0 for k in KC.FUZZ_KINDS}
    for seed in range(240):
        kind, pts = KC.fuzz_cloud(seed)
        out, fin, _ = KC.host_dist2(lib, pts)
        assert (fin >= 0).all()
        w = KC.worst_ratio(out, KC.oracle_rows(pts, np.arange(len(pts))))
        assert w <= 1.0, (seed, kind, len(pts), w)
        worst[kind] = max(worst[kind], w)
    print("knn host fuzz, worst error / bound per kind:", {k: round(v, 3) for k, v in worst.items()})


def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "knn_host_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DKNN_MAIN", "-I", KC.CSRC, KC.SRC, "-o", exe], check=True)
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        f.write(np.array([len(KC.NAMES)], np.int32).tobytes())
        for name in KC.NAMES:
            pts = KC.points(name)
            f.write(np.array([len(pts)], np.int32).tobytes())
            f.write(pts.tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"cases {len(KC.NAMES)}"
    for k, name in enumerate(KC.NAMES):   # the same answers as the library the other tests load
        out, fin, dims = KC.host_result(name)
        want = (f"case {k} P {len(out)} dims {dims[0]} {dims[1]} {dims[2]} fallback {int((fin & KC.FIN_FALLBACK != 0).sum())} "
                f"whole {int((fin & KC.FIN_WHOLE != 0).sum())} shell {int((fin & KC.FIN_SHELL).max())} hash {KC.fnv1a(out)}")
        assert lines[k] == want, name


# ---- the CPU branch of simple_knn._C ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p1", "p2", "p3", "p4", "p5", "p7"])
def test_cpu_branch_follows_the_contract(name):
    from simple_knn._C import distCUDA2
    got = distCUDA2(torch.from_numpy(KC.points(name).copy()))
    assert got.dtype == torch.float32 and got.shape == (len(KC.points(name)),)
    KC.check("cpu branch", name, got.numpy(), KC.oracle(name))


def test_cpu_branch_empty():
    from simple_knn._C import distCUDA2
    assert distCUDA2(torch.zeros(0, 3)).shape == (0,)

"""gsr_knn_query's and gsr_knn_gather_mean's scalar source (csrc/gsr_knnq.h) on the CPU: tests/host_math/knnq_host.cpp runs
the device pipeline's steps in plain loops over the header the kernels compile.  The result must EQUAL oracle E of
tests/knnq_cases.py on every named case -- indices and the bits of d2 --, the finish codes prove which path each case takes,
the mean is held to oracle M, a stand-alone build runs the cases under the address and undefined-behaviour sanitizers, and the
CPU branch of diff_gaussian_rasterization.knn_ops gives the same answers.  No GPU."""
import numpy as np
import pytest
import torch

import knnq_cases as QC


@pytest.fixture(scope="module")
def lib():
    return QC.host_lib()


@pytest.mark.parametrize("name", QC.NAMES)
def test_host_build_equals_oracle(lib, name):
    idx, d2, fin, dims = QC.host_result(name)
    assert (fin >= 0).all(), "queries the search never wrote"
    QC.check_exact("host", name, idx, d2)


def test_contract_in_numbers(lib):
    """missing slots, the index rule, exclusion and non-finite points, spelled out on the smallest cases"""
    idx, d2, _, _ = QC.host_result("r0-q65")
    assert (idx == -1).all() and np.isposinf(d2).all()                          # no reference: every slot missing
    idx, d2, _, _ = QC.host_result("r2-q63")
    assert (idx[:, :2] >= 0).all() and (idx[:, 2:] == -1).all() and np.isposinf(d2[:, 2:]).all()
    assert (d2[:, 0] <= d2[:, 1]).all()
    idx, d2, _, _ = QC.host_result("twopos")                                    # 255 coincident points: ties by index
    assert np.array_equal(idx[:255], np.tile(np.arange(5, dtype=np.int32), (255, 1))) and (d2[:255] == 0).all()
    idx, _, _, _ = QC.host_result("twopos-self")                                # ... and without the query's own index
    for q in (0, 3, 254):
        assert np.array_equal(idx[q], np.array([i for i in range(9) if i != q][:8], np.int32))
    idx, _, _, _ = QC.host_result("uniform-same")                               # queries = references: rank 0 is the point
    assert np.array_equal(idx[:, 0], np.arange(len(idx), dtype=np.int32))
    idx3, _, _, _ = QC.host_result("uniform-self3")
    assert not (idx3 == np.arange(len(idx3))[:, None]).any()
    assert np.array_equal(idx[:, 1:], idx3[:, :2])
    for name, at in (("nan-point-self", QC.KC.NAN_AT[0]), ("inf-point-self", QC.KC.INF_AT[0])):
        idx, d2, fin, _ = QC.host_result(name)
        assert (idx[at] == -1).all() and np.isposinf(d2[at]).all() and fin[at] == QC.FIN_NONFINITE
        assert not (idx == at).any()                                            # invisible to every query
    for name in ("nan-query", "inf-query"):
        idx, d2, fin, _ = QC.host_result(name)
        assert (idx[[13, 40]] == -1).all() and (fin[[13, 40]] == QC.FIN_NONFINITE).all()
        assert (np.delete(idx, [13, 40], axis=0) >= 0).all()


def test_refusals(lib):
    p = np.zeros((4, 3), np.float32)
    out = np.zeros((4, 8), np.int32)
    fin, dims = np.zeros(4, np.int32), np.zeros(3, np.int32)
    def call(R, Q, k, flags):
        return lib.kq_query(p.ctypes.data, R, p.ctypes.data, Q, k, flags, out.ctypes.data, None, fin.ctypes.data, dims.ctypes.data)
    assert call(4, 4, 3, 0) == 0
    assert call(4, 4, 0, 0) == 1 and call(4, 4, 9, 0) == 1 and call(-1, 4, 3, 0) == 1 and call(4, -1, 3, 0) == 1
    assert call(4, 4, 3, 2) == 1 and call(4, 3, 3, QC.EXCLUDE) == 1


def test_cases_take_the_paths_they_claim():
    seen = dict(shell0=[], later=[], whole=[], fallback=[], outside=[], nonfinite=[])
    for name in QC.NAMES:
        idx, _, fin, dims = QC.host_result(name)
        if len(fin) == 0 or QC.case(name)[0].shape[0] == 0:
            continue
        live = fin[(fin & QC.FIN_NONFINITE) == 0]
        plain = (live & (QC.FIN_WHOLE | QC.FIN_FALLBACK)) == 0
        shell = live & QC.FIN_SHELL
        counts = dict(shell0=int((plain & (shell == 0)).sum()), later=int((plain & (shell > 0)).sum()),
                      whole=int(((live & QC.FIN_WHOLE) != 0).sum()), fallback=int(((live & QC.FIN_FALLBACK) != 0).sum()),
                      outside=int(((live & QC.FIN_OUTSIDE) != 0).sum()), nonfinite=int(((fin & QC.FIN_NONFINITE) != 0).sum()))
        print(f"knnq paths {name}: R {QC.case(name)[0].shape[0]} Q {len(fin)} dims {dims} {counts}")
        assert not (((live & QC.FIN_FALLBACK) != 0) & ((live & QC.FIN_WHOLE) != 0)).any()
        for key, n in counts.items():
            if n:
                seen[key].append(name)
        if name in QC.ONE_CELL:
            assert dims == (1, 1, 1) and counts["whole"] == len(live), (name, dims, counts)
    # the cases that are there FOR a path take it
    assert "uniform-self3" in seen["shell0"] and "clusters" in seen["later"]
    assert "p2" in seen["whole"] and "twopos" in seen["whole"]
    assert seen["fallback"] and set(seen["fallback"]) >= {"slabs"}
    fin = QC.host_result("slabs")[2]
    assert ((fin & QC.FIN_FALLBACK) != 0).sum() >= 3                # the middle points need more than MAX_SHELL shells
    fin = QC.host_result("outside")[2]
    assert ((fin & QC.FIN_OUTSIDE) != 0).all()                       # every query of 'outside' has a clamped cell
    assert QC.host_result("line")[3] == (256, 2, 2)                  # the cap
    assert {"nan-query", "inf-query", "nan-point-self", "inf-point-self"} <= set(seen["nonfinite"])


def test_mean_against_oracle_and_rank_order(lib):
    idx, tensors = QC.mean_inputs()
    for name, t in tensors.items():
        got = QC.host_gather_mean(lib, idx, t)
        QC.check_mean("host " + name, got, idx, t.reshape(len(t), -1))
        assert (got[7] == 0).all()                                            # a row of -1 gives zeros
    # the float32 sum in rank order, then one division: spelled out for one row
    t = tensors["xyz"]
    got = QC.host_gather_mean(lib, idx, t)
    acc = t[idx[0, 0]].copy()
    for r in range(1, idx.shape[1]):
        acc = (acc + t[idx[0, r]]).astype(np.float32)
    assert np.array_equal(got[0], (acc / np.float32(idx.shape[1])).astype(np.float32))
    assert np.array_equal(got[11], ((t[idx[11, 0]] + t[idx[11, 2]] + t[idx[11, 3]] + t[idx[11, 4]]) / np.float32(4)).astype(np.float32))


def _fnv1a(*arrays):
    h = 2166136261
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 16777619) & 0xffffffff
    return h


def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    import os
    import subprocess
    src = os.path.join(QC.KC.HM, "knnq_host.cpp")
    exe = str(tmp_path / "knnq_host_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DKNNQ_MAIN", "-I", QC.KC.CSRC, src, "-o", exe], check=True)
    names = [n for n in QC.NAMES if QC.case(n)[0].shape[0] * QC.case(n)[1].shape[0] <= 5_000_000]     # (the hash loop is Python)
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        f.write(np.array([len(names)], np.int32).tobytes())
        for name in names:
            ref, qry, k, flags = QC.case(name)
            f.write(np.array([len(ref), len(qry), k, flags], np.int32).tobytes())
            f.write(ref.tobytes())
            f.write(qry.tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"cases {len(names)}"
    for c, name in enumerate(names):      # the same answers as the library the other tests load
        idx, d2, fin, dims = QC.host_result(name)
        want = f"case {c} R {len(QC.case(name)[0])} Q {len(idx)} k {idx.shape[1]} dims {dims[0]} {dims[1]} {dims[2]} hash {_fnv1a(idx, d2, fin)}"
        assert lines[c] == want, name


# ---- the CPU branch of knn_ops ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in QC.NAMES if QC.case(n)[0].shape[0] * QC.case(n)[1].shape[0] <= 5_000_000])  # (the
# branch sorts all R distances of every query: the 6000 x 6000 self-queries are left to the host build)
def test_cpu_branch_equals_oracle(name):
    from diff_gaussian_rasterization import knn_ops
    ref, qry, k, flags = QC.case(name)
    idx, d2 = knn_ops.knn_query(torch.from_numpy(ref.copy()), torch.from_numpy(qry.copy()), k=k, exclude_self=bool(flags & QC.EXCLUDE))
    QC.check_exact("cpu branch", name, idx.numpy(), d2.numpy())


def test_cpu_branch_self_query_default_and_refusals():
    from diff_gaussian_rasterization import knn_ops
    ref = torch.from_numpy(QC.case("self7-k3")[0].copy())
    idx, d2 = knn_ops.knn_query(ref)                                              # qry=None: k = 3, exclusion
    QC.check_exact("cpu branch default", "self7-k3", idx.numpy(), d2.numpy())
    for bad_k in (0, 9):
        with pytest.raises(ValueError):
            knn_ops.knn_query(ref, k=bad_k)
    with pytest.raises(ValueError):
        knn_ops.knn_query(ref, ref[:3], k=2, exclude_self=True)


def test_cpu_branch_mean_equals_host_build(lib):
    from diff_gaussian_rasterization import knn_ops
    idx, tensors = QC.mean_inputs()
    names = list(tensors)
    got = knn_ops.gather_mean(torch.from_numpy(idx), [torch.from_numpy(tensors[n]) for n in names])
    for n, g in zip(names, got):
        assert g.shape == (idx.shape[0],) + tensors[n].shape[1:] and g.dtype == torch.float32
        want = QC.host_gather_mean(lib, idx, tensors[n])
        assert np.array_equal(g.numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32)), n

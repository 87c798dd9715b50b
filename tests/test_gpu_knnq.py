"""gsr_knn_query and gsr_knn_gather_mean on the device (csrc/gsr_knnq.hip.h) and what stands on them: the result EQUALS
oracle E of tests/knnq_cases.py on every named case (indices and the bits of d2) and the host build of the same scalar source;
the k = 3 self-query agrees with distCUDA2; repeats and a side stream give the same bits; nothing is written outside the
outputs; the gather-mean matches oracle M and the host build's knnq_mean bit for bit; GaussianModel.inpaint_setup on the
device gives the CPU path's rows; fill_group renders; and one plausibility run at R = 1 000 000."""
import ctypes

import numpy as np
import pytest
import torch

import knn_cases as KC
import knnq_cases as QC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _query(dev, ref, qry, k, flags):
    from diff_gaussian_rasterization import knn_ops
    r = torch.from_numpy(ref.copy()).to(dev)
    q = r if qry is ref else torch.from_numpy(qry.copy()).to(dev)
    idx, d2 = knn_ops.knn_query(r, q, k=k, exclude_self=bool(flags & QC.EXCLUDE))
    return idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("name", QC.NAMES)
def test_device_equals_oracle_and_host_build(dev, name):
    ref, qry, k, flags = QC.case(name)
    idx, d2 = _query(dev, ref, qry, k, flags)
    QC.check_exact("device", name, idx, d2)
    h_idx, h_d2, _, _ = QC.host_result(name)
    QC.check_exact("device vs host build", name, idx, d2, want=(h_idx, h_d2))


def test_self_query_agrees_with_distcuda2(dev):
    from diff_gaussian_rasterization import knn_ops
    from simple_knn._C import distCUDA2
    for name in ("uniform", "clusters", "outliers"):
        pts = torch.from_numpy(KC.points(name).copy()).to(dev)
        idx, d2 = knn_ops.knn_query(pts)                               # qry=None: k = 3, exclusion
        assert idx.shape == (len(pts), 3) and not (idx == torch.arange(len(pts), device=dev)[:, None]).any()
        mean = ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / 3.0
        w = KC.worst_ratio(mean.cpu().numpy(), distCUDA2(pts).cpu().numpy().astype(np.float64))
        print(f"knnq self-query vs distCUDA2 {name}: worst difference / bound {w:.3f}")
        assert w <= 1.0, (name, w)


def test_repeat_and_side_stream_give_the_same_bits(dev):
    from diff_gaussian_rasterization import knn_ops
    ref, qry, k, flags = QC.case("clusters")
    r, q = torch.from_numpy(ref.copy()).to(dev), torch.from_numpy(qry.copy()).to(dev)
    _, tensors = QC.mean_inputs(R=len(ref))
    src = [torch.from_numpy(t).to(dev) for t in tensors.values()]
    idx0, d20 = knn_ops.knn_query(r, q, k=k)
    m0 = knn_ops.gather_mean(idx0, src)
    idx1, d21 = knn_ops.knn_query(r, q, k=k)
    m1 = knn_ops.gather_mean(idx1, src)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        idx2, d22 = knn_ops.knn_query(r, q, k=k)
        m2 = knn_ops.gather_mean(idx2, src)
    side.synchronize()
    for i, d, m in ((idx1, d21, m1), (idx2, d22, m2)):
        assert torch.equal(i, idx0) and torch.equal(d.view(torch.int32), d20.view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(m, m0))


@pytest.mark.parametrize("Q", [1, 65])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_nothing_is_written_outside_the_outputs(dev, Q, k):
    import diff_gaussian_rasterization as D
    lib = D._load()
    PAD = 256
    r = np.random.default_rng(Q * 10 + k)
    ref = torch.from_numpy(r.random((300, 3), dtype=np.float32)).to(dev)
    qry = torch.from_numpy(r.random((Q, 3), dtype=np.float32)).to(dev)
    out_idx = torch.full((PAD + Q * k + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    out_d2 = torch.full((PAD + Q * k + PAD,), -123.0, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gsr_knn_query(ref.data_ptr(), 300, qry.data_ptr(), Q, k, 0, out_idx.data_ptr() + 4 * PAD, out_d2.data_ptr() + 4 * PAD,
                               D._stream(dev))
    assert rc == 0, D._err(lib)
    idx = out_idx[PAD:PAD + Q * k].reshape(Q, k)
    d2 = out_d2[PAD:PAD + Q * k].reshape(Q, k)
    want = QC.oracle_e(ref.cpu().numpy(), qry.cpu().numpy(), k)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    for buf, fill in ((out_idx, 0x5A5A5A5A), (out_d2, -123.0)):
        assert (buf[:PAD] == fill).all() and (buf[PAD + Q * k:] == fill).all()
    # without out_d2, and the gather-mean's destinations
    out_idx.fill_(0x5A5A5A5A)
    with torch.cuda.device(dev):
        rc = lib.gsr_knn_query(ref.data_ptr(), 300, qry.data_ptr(), Q, k, 0, out_idx.data_ptr() + 4 * PAD, None, D._stream(dev))
    assert rc == 0 and torch.equal(out_idx[PAD:PAD + Q * k].reshape(Q, k), idx.clone())
    assert (out_idx[:PAD] == 0x5A5A5A5A).all() and (out_idx[PAD + Q * k:] == 0x5A5A5A5A).all()
    cols = (3, 45, 1, 16)
    srcs = [torch.from_numpy(r.standard_normal((300, c)).astype(np.float32)).to(dev) for c in cols]
    dsts = [torch.full((PAD + Q * c + PAD,), -123.0, dtype=torch.float32, device=dev) for c in cols]
    src_a = (ctypes.c_void_p * 4)(*[s.data_ptr() for s in srcs])
    dst_a = (ctypes.c_void_p * 4)(*[d.data_ptr() + 4 * PAD for d in dsts])
    col_a = (ctypes.c_int32 * 4)(*cols)
    idx_c = idx.contiguous()
    with torch.cuda.device(dev):
        rc = lib.gsr_knn_gather_mean(idx_c.data_ptr(), Q, k, 300, 4, src_a, col_a, dst_a, D._stream(dev))
    assert rc == 0, D._err(lib)
    for s, d, c in zip(srcs, dsts, cols):
        assert (d[:PAD] == -123.0).all() and (d[PAD + Q * c:] == -123.0).all()
        QC.check_mean(f"padded Q={Q} k={k} cols={c}", d[PAD:PAD + Q * c].reshape(Q, c).cpu().numpy(), idx_c.cpu().numpy(), s.cpu().numpy())


def test_gather_mean_against_oracle_and_host_build(dev):
    from diff_gaussian_rasterization import knn_ops
    lib = QC.host_lib()
    for k in (1, 5, 8):
        idx, tensors = QC.mean_inputs(k=k, seed=k)
        names = list(tensors)
        got = knn_ops.gather_mean(torch.from_numpy(idx).to(dev), [torch.from_numpy(tensors[n]).to(dev) for n in names])
        for n, g in zip(names, got):
            assert g.shape == (idx.shape[0],) + tensors[n].shape[1:] and g.dtype == torch.float32
            g = g.cpu().numpy().reshape(idx.shape[0], -1)
            QC.check_mean(f"device k={k} {n}", g, idx, tensors[n].reshape(len(tensors[n]), -1))
            want = QC.host_gather_mean(lib, idx, tensors[n])
            assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (k, n)       # the same bits as knnq_mean on the host
            assert (g[7] == 0).all()                                                     # a row of -1 gives zeros
    # more than one call's worth of tensors and columns (9 tensors; 128 + 128 columns)
    r = np.random.default_rng(5)
    idx = r.integers(-1, 50, (40, 5)).astype(np.int32)
    many = [r.standard_normal((50, c)).astype(np.float32) for c in (1, 2, 3, 4, 5, 6, 7, 8, 9, 128, 128)]
    got = knn_ops.gather_mean(torch.from_numpy(idx).to(dev), [torch.from_numpy(t).to(dev) for t in many])
    for t, g in zip(many, got):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), QC.host_gather_mean(lib, idx, t).view(np.uint32))
    with pytest.raises(ValueError):
        knn_ops.gather_mean(torch.from_numpy(idx).to(dev), [torch.zeros(50, 129, device=dev)])


def test_inpaint_setup_on_the_device_equals_the_cpu_path(dev):
    import os
    from gsplat_attack.gaussian_model import GaussianModel
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_inpaint.npz"))
    attrs = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_objects_dc")
    t = [torch.from_numpy(z["in/" + n].copy()) for n in attrs]
    mask = torch.from_numpy(z["mask"].copy())
    for m_removed, k in ((mask, 5), (mask, 8), (torch.arange(400) >= 3, 5)):          # the last: 3 remain, fewer than k
        cpu = GaussianModel.from_tensors(t[0], t[1], t[2], t[3], t[4], t[5], t[6])
        gpu = GaussianModel.from_tensors(t[0], t[1], t[2], t[3], t[4], t[5], t[6], device=dev)
        new_c = cpu.inpaint_setup(m_removed, k=k)
        new_g = gpu.inpaint_setup(m_removed.to(dev), k=k)
        assert new_g.device.type == "cuda" and torch.equal(new_g.cpu(), new_c)
        for n in attrs:
            a, b = getattr(gpu, n), getattr(cpu, n)
            assert isinstance(a, torch.nn.Parameter) and a.requires_grad and a.device.type == "cuda"
            assert torch.equal(a.detach().cpu().view(torch.int32), b.detach().view(torch.int32)), (n, k)   # bit for bit
    with pytest.raises(ValueError, match="remains"):
        gpu.inpaint_setup(torch.ones(gpu._xyz.shape[0], dtype=torch.bool, device=dev))


def test_fill_group_then_render(dev):
    from gsplat_attack.groups import fill_group, select_group
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene, synthetic_grouping
    model, cams, _ = make_scene("nyc-1M", device=dev, P=100_000, width=320, height=192, n_views=1)
    xyz = model._xyz.detach()
    middle = ((xyz[:, 0].abs() < 8) & (xyz[:, 1].abs() < 8) & (xyz[:, 2] > 0.5)).cpu()
    sd = synthetic_grouping(model, middle, 42)
    mask3d, _ = select_group(model, sd, [42])
    removed = int(mask3d.sum())
    assert 0 < removed < model._xyz.shape[0]
    P0 = model._xyz.shape[0]
    filled, new_mask = fill_group(model, mask3d, k=5)
    assert model._xyz.shape[0] == P0 and filled._xyz.shape[0] == P0                 # one new row per removed one
    assert int(new_mask.sum()) == removed and bool(new_mask[P0 - removed:].all())
    assert torch.equal(filled._xyz.detach()[:P0 - removed], model._xyz.detach()[~mask3d])
    out = render(cams[0], filled, PipelineParams(skip_objects=True), torch.zeros(3, device=dev))
    img = out["render"]
    assert torch.isfinite(img).all() and float(img.detach().abs().sum()) > 0
    img.sum().backward()
    for n in ("_xyz", "_features_dc", "_scaling", "_rotation", "_opacity"):
        g = getattr(filled, n).grad
        assert g is not None and torch.isfinite(g).all(), n
    assert float(filled._xyz.grad[new_mask].abs().sum()) > 0                         # the new rows are seen and trainable


def test_one_million_references_spot_checked(dev):
    from diff_gaussian_rasterization import knn_ops
    from gsplat_attack.scenes import city
    xyz = city(1_050_000, 7, 20.0, 60)["xyz"].float().contiguous()
    ref, qry = xyz[:1_000_000].to(dev), xyz[1_000_000:].to(dev)
    k = 5
    idx, d2 = knn_ops.knn_query(ref, qry, k=k)
    assert idx.shape == (50_000, k) and int(idx.min()) >= 0 and int(idx.max()) < 1_000_000
    assert bool((d2[:, 1:] >= d2[:, :-1]).all())
    rows = torch.from_numpy(np.random.default_rng(1).choice(50_000, 200, replace=False)).to(dev)
    r64 = ref.double()
    for s in range(0, 200, 50):                                                      # oracle E on the device, in float64
        rr = rows[s:s + 50]
        q = qry[rr].double()
        dx, dy, dz = (r64[None, :, a] - q[:, None, a] for a in range(3))
        e = (dx * dx + dy * dy) + dz * dz
        thr = torch.topk(e, k, dim=1, largest=False).values[:, -1:]
        for i in range(len(rr)):
            cand = torch.nonzero(e[i] <= thr[i]).flatten()                           # ascending index
            cd = e[i][cand].cpu().numpy()
            order = np.lexsort((cand.cpu().numpy(), cd))[:k]
            assert np.array_equal(idx[rr[i]].cpu().numpy(), cand.cpu().numpy()[order].astype(np.int32)), int(rr[i])
            assert np.array_equal(d2[rr[i]].cpu().numpy().view(np.uint32), cd[order].astype(np.float32).view(np.uint32)), int(rr[i])

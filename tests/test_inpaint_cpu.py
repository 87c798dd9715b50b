"""GaussianModel.inpaint_setup on CPU tensors against tests/golden/ref_inpaint.npz -- the reference's own inpaint_setup
(scene/gaussian_model.py:264-348), executed by tests/golden/make_golden_inpaint.py on a 400-Gaussian model with 60 rows
masked --, the stated deviations from the reference, and gsplat_attack.groups.fill_group.  No GPU: the CPU branch of
diff_gaussian_rasterization.knn_ops evaluates the same definition as the kernels."""
import os

import numpy as np
import pytest
import torch

import knnq_cases as QC

HERE = os.path.dirname(os.path.abspath(__file__))
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_objects_dc")


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(HERE, "golden", "ref_inpaint.npz"))
    return {k: z[k] for k in z.files}


def _model(gold):
    from gsplat_attack.gaussian_model import GaussianModel
    t = {n: torch.from_numpy(gold["in/" + n].copy()) for n in ATTRS}
    return GaussianModel.from_tensors(t["_xyz"], t["_features_dc"], t["_features_rest"], t["_scaling"], t["_rotation"], t["_opacity"],
                                      t["_objects_dc"])


def test_fixture_is_what_the_generator_promises(gold):
    assert gold["mask"].shape == (400,) and int(gold["mask"].sum()) == 60 and int(gold["k"]) == 5
    assert float(gold["min_relative_gap"]) > 1e-5                 # no tie that KDTree could have decided otherwise
    for n in ATTRS:
        assert gold["out/" + n].shape == gold["in/" + n].shape and bool(gold["out_requires_grad/" + n])


def test_inpaint_setup_reproduces_the_reference(gold):
    m = _model(gold)
    mask = torch.from_numpy(gold["mask"].copy())
    new_mask = m.inpaint_setup(mask, k=int(gold["k"]))
    keep = ~gold["mask"]
    n_keep, n_new = int(keep.sum()), int(gold["mask"].sum())
    assert new_mask.dtype == torch.bool and new_mask.shape == (400,)
    assert not new_mask[:n_keep].any() and new_mask[n_keep:].all() and int(new_mask.sum()) == n_new
    # the neighbour sets, exactly: oracle E on the fixture's positions must be what the reference's rows are the means of
    rest_xyz, qry_xyz = gold["in/_xyz"][keep], gold["in/_xyz"][gold["mask"]]
    idx, _ = QC.oracle_e(rest_xyz, qry_xyz, int(gold["k"]))
    from diff_gaussian_rasterization import knn_ops
    got_idx, _ = knn_ops.knn_query(torch.from_numpy(rest_xyz.copy()), torch.from_numpy(qry_xyz.copy()), k=int(gold["k"]), exclude_self=False)
    assert np.array_equal(got_idx.numpy(), idx)
    for n in ATTRS:
        got = getattr(m, n)
        assert isinstance(got, torch.nn.Parameter) and got.requires_grad and got.is_leaf
        got = got.detach().numpy()
        ref = gold["out/" + n]
        assert got.shape == ref.shape and got.dtype == np.float32
        assert np.array_equal(got[:n_keep].view(np.uint32), gold["in/" + n][keep].view(np.uint32)), n      # remaining rows: bit-equal, in order
        assert np.array_equal(ref[:n_keep], gold["in/" + n][keep]), n
        # new rows: ours and the reference's are both within oracle M's bound of the float64 mean over OUR neighbour sets --
        # which the reference's rows can only be if its sets are the same: another neighbour moves a mean by a fifth of the
        # difference of two random rows, orders of magnitude above 2^-23 of their magnitudes
        src = gold["in/" + n][keep].reshape(n_keep, -1)
        QC.check_mean("inpaint " + n, got[n_keep:].reshape(n_new, -1), idx, src)
        QC.check_mean("reference " + n, ref[n_keep:].reshape(n_new, -1), idx, src)


def test_fewer_than_k_remaining_are_averaged_as_they_are(gold):
    m = _model(gold)
    P = m._xyz.shape[0]
    mask = torch.ones(P, dtype=torch.bool)
    mask[[5, 17, 300]] = False                                     # three remain, k = 5
    before = {n: getattr(m, n).detach().clone() for n in ATTRS}
    new_mask = m.inpaint_setup(mask, k=5)
    assert m._xyz.shape[0] == P and int(new_mask.sum()) == P - 3
    for n in ATTRS:
        rest = before[n][[5, 17, 300]]
        assert torch.equal(getattr(m, n).detach()[:3], rest)
        new = getattr(m, n).detach()[3:].reshape(P - 3, -1).numpy().astype(np.float64)
        want = rest.reshape(3, -1).numpy().astype(np.float64).mean(axis=0)
        bound = QC.MEAN_BOUND * np.abs(rest.reshape(3, -1).numpy().astype(np.float64)).sum(axis=0)
        assert (np.abs(new - want) <= bound).all(), n              # every new row: the mean of the three, in some rank order


def test_none_remaining_raises_and_an_all_false_mask_adds_nothing(gold):
    m = _model(gold)
    P = m._xyz.shape[0]
    with pytest.raises(ValueError, match="remains"):
        m.inpaint_setup(torch.ones(P, dtype=torch.bool))
    assert m._xyz.shape[0] == P                                    # untouched by the refused call
    before = {n: getattr(m, n).detach().clone() for n in ATTRS}
    new_mask = m.inpaint_setup(torch.zeros(P, dtype=torch.bool))
    assert new_mask.shape == (P,) and not new_mask.any()
    for n in ATTRS:
        got = getattr(m, n)
        assert isinstance(got, torch.nn.Parameter) and got.requires_grad and torch.equal(got.detach(), before[n])
    with pytest.raises(ValueError, match="mask of"):
        m.inpaint_setup(torch.zeros(P - 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        m.inpaint_setup(torch.from_numpy(gold["mask"].copy()), k=9)
    with pytest.raises(TypeError):                                 # the reference's unread thresholds are accepted nowhere
        m.inpaint_setup(torch.zeros(P, dtype=torch.bool), distance_threshold=0.25)


def test_mask_semantics_and_requires_grad(gold):
    """mask3d selects the rows to REMOVE, in any shape the reference's .squeeze() takes and any dtype .bool() takes; frozen
    inputs come back as trainable Parameters (nn.Parameter's default wins, as in removal_setup)"""
    from gsplat_attack.gaussian_model import GaussianModel
    ref = _model(gold)
    mask = torch.from_numpy(gold["mask"].copy())
    ref.inpaint_setup(mask)
    t = {n: torch.from_numpy(gold["in/" + n].copy()) for n in ATTRS}
    frozen = GaussianModel.from_tensors(t["_xyz"], t["_features_dc"], t["_features_rest"], t["_scaling"], t["_rotation"], t["_opacity"],
                                        t["_objects_dc"], requires_grad=False)
    frozen.inpaint_setup(mask.to(torch.uint8)[:, None])
    for n in ATTRS:
        assert getattr(frozen, n).requires_grad and torch.equal(getattr(frozen, n).detach(), getattr(ref, n).detach())


def test_fill_group_works_on_a_clone(gold):
    from gsplat_attack.groups import fill_group
    m = _model(gold)
    before = {n: getattr(m, n) for n in ATTRS}
    mask = torch.from_numpy(gold["mask"].copy())
    filled, new_mask = fill_group(m, mask, k=5)
    for n in ATTRS:
        assert getattr(m, n) is before[n]                           # the model itself is untouched
    direct = _model(gold)
    direct_mask = direct.inpaint_setup(mask, k=5)
    assert torch.equal(new_mask, direct_mask)
    for n in ATTRS:
        assert torch.equal(getattr(filled, n).detach(), getattr(direct, n).detach())
    with pytest.raises(ValueError, match="mask of"):
        fill_group(m, mask[:-1])

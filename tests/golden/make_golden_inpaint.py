"""Generate tests/golden/ref_inpaint.npz by EXECUTING the reference's own inpaint_setup (scene/gaussian_model.py:264-367) on
the CPU: a 400-Gaussian random model (raw parameters written here), 60 rows masked.

The reference finds, for every masked Gaussian, the 5 nearest remaining ones with scipy's KDTree, appends the numpy mean of
their rows for each of the seven attribute tensors, and assigns the seven nn.Parameters (:342-348).  Its next line (:351)
asks for device "cuda" and raises on a machine without one; by then the parameters are assigned, so the exception is caught
and the parameters are stored.

Ties.  KDTree's choice among equidistant neighbours is arbitrary and its distances are float64 roundings of another
expression than ours.  So that neither can reorder anything, the script computes, over all queries, the smallest relative gap
between consecutive neighbour distances up to rank k + 1 (float64 brute force), stores it, and REFUSES to write the fixture
unless it exceeds 1e-5.

Run where the reference is available (it never travels with the repository):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_inpaint.py

Third-party modules this image lacks (plyfile, simple_knn) are empty stand-ins for the import only.  Data only: inputs
written by this script, outputs produced by the reference's code.  The fixture holds arrays only.
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_objects_dc")
P, N_MASKED, K = 400, 60, 5


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    _stub("plyfile", PlyData=object, PlyElement=object)
    _stub("simple_knn")
    _stub("simple_knn._C", distCUDA2=None)
    from scene.gaussian_model import GaussianModel

    gen = torch.Generator().manual_seed(2718)
    raw = dict(_xyz=torch.randn(P, 3, generator=gen) * 2.0, _features_dc=torch.randn(P, 1, 3, generator=gen),
               _features_rest=torch.randn(P, 15, 3, generator=gen) * 0.2, _scaling=torch.randn(P, 3, generator=gen) - 3.0,
               _rotation=torch.randn(P, 4, generator=gen), _opacity=torch.randn(P, 1, generator=gen),
               _objects_dc=torch.randn(P, 1, 16, generator=gen))
    mask = torch.zeros(P, dtype=torch.bool)
    mask[torch.randperm(P, generator=gen)[:N_MASKED]] = True

    # ---- the gap between consecutive neighbour distances, ranks 1 .. k + 1 ------------------------------------------------
    xyz = raw["_xyz"].numpy().astype(np.float64)
    rest, qry = xyz[~mask.numpy()], xyz[mask.numpy()]
    d = np.sqrt(((qry[:, None, :] - rest[None, :, :]) ** 2).sum(axis=2))
    near = np.sort(d, axis=1)[:, :K + 1]
    gap = float(((near[:, 1:] - near[:, :-1]) / near[:, 1:]).min())
    print(f"smallest relative gap between consecutive neighbour distances up to rank {K + 1}: {gap:.3e}")
    assert gap > 1e-5, "neighbour distances too close to a tie: choose another seed"

    pc = GaussianModel(3)
    for n, v in raw.items():
        setattr(pc, n, torch.nn.Parameter(v.clone().requires_grad_(True)))
    args = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1e-4, feature_lr=1e-3, opacity_lr=1e-2, scaling_lr=1e-3,
                                 rotation_lr=1e-3)
    raised = None
    try:
        pc.inpaint_setup(args, mask)
    except Exception as e:       # scene/gaussian_model.py:351, device="cuda": after the seven parameters are assigned
        raised = e
    assert raised is not None and pc._xyz.shape[0] == P, (raised, pc._xyz.shape)
    print("the reference stopped at:", type(raised).__name__, str(raised).splitlines()[0][:100])

    out = {"mask": mask.numpy(), "k": np.array(K), "min_relative_gap": np.array(gap)}
    for n, v in raw.items():
        out["in/" + n] = v.numpy()
        got = getattr(pc, n)
        assert isinstance(got, torch.nn.Parameter) and got.shape == v.shape
        out["out/" + n] = got.detach().numpy()
        out["out_requires_grad/" + n] = np.array(bool(got.requires_grad))
    path = os.path.join(HERE, "ref_inpaint.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

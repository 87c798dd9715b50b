"""The groups set-up's entry points (C ABI 603): exported, their argument checks answer before any device call, the host
hull runs without a device, and both classifier state-dict layouts load.  This file runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsr_group_classify", "gsr_convex_hull_planes", "gsr_points_in_hull")
GSR_ERR_INVALID, GSR_ERR_NOMEM = 1, 3


@pytest.fixture(scope="module")
def lib():
    import diff_gaussian_rasterization as D
    if not os.path.exists(D.library_path()):
        import __graft_entry__
        __graft_entry__.build()
    from diff_gaussian_rasterization import groups
    return groups._lib()


def _err(lib):
    return lib.gsr_last_error().decode()


def test_symbols_exported_and_version(lib):
    text = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n + "(" in text, f"{n} not declared in include/gsraster.h"
    out = ctypes.c_int64(0)
    assert lib.gsr_query(0, ctypes.byref(out)) == 0 and out.value >= 603


def _ids(*v):
    a = (ctypes.c_int32 * len(v))(*v)
    return a, len(v)


def test_classify_argument_checks(lib):
    one = ctypes.c_void_p(256)
    f = lib.gsr_group_classify
    ids, n = _ids(3)
    for C in (0, 1025):
        assert f(one, 10, one, one, C, ids, n, 0.5, one, one, None) == GSR_ERR_INVALID and "C=" in _err(lib)
    assert f(one, 10, one, one, 8, None, 1, 0.5, one, one, None) == GSR_ERR_INVALID and "ids" in _err(lib)
    assert f(one, 10, one, one, 8, ids, 0, 0.5, one, one, None) == GSR_ERR_INVALID
    dup, n = _ids(1, 5, 1)
    assert f(one, 10, one, one, 8, dup, n, 0.5, one, one, None) == GSR_ERR_INVALID and "duplicate id 1" in _err(lib)
    for bad in (-1, 8):
        b, n = _ids(2, bad)
        assert f(one, 10, one, one, 8, b, n, 0.5, one, one, None) == GSR_ERR_INVALID and f"id {bad} outside" in _err(lib)
    ok, n = _ids(0, 7)
    for k in (0, 2, 3, 8, 9):                                     # each device pointer null in turn
        a = [one, 10, one, one, 8, ok, n, 0.5, one, one, None]
        a[k] = None
        assert f(*a) == GSR_ERR_INVALID and "null" in _err(lib)
    assert f(one, -1, one, one, 8, ok, n, 0.5, one, one, None) == GSR_ERR_INVALID
    assert f(one, 10, one, one, 8, ok, n, float("nan"), one, one, None) == GSR_ERR_INVALID
    assert f(None, 0, None, None, 8, ok, n, 0.5, None, None, None) == 0        # P = 0: nothing to do, no device touched


def test_points_in_hull_argument_checks(lib):
    one = ctypes.c_void_p(256)
    f = lib.gsr_points_in_hull
    assert f(one, 10, one, -1, one, 0.0, None, one, None) == GSR_ERR_INVALID and "F=-1" in _err(lib)
    assert f(one, -3, one, 4, one, 0.0, None, one, None) == GSR_ERR_INVALID
    for k in (0, 4, 7):
        a = [one, 10, one, 4, one, 0.0, None, one, None]
        a[k] = None
        assert f(*a) == GSR_ERR_INVALID and "null" in _err(lib)
    assert f(one, 10, None, 4, one, 0.0, None, one, None) == GSR_ERR_INVALID
    assert f(one, 10, one, 4, one, -1.0, None, one, None) == GSR_ERR_INVALID and "tau" in _err(lib)
    assert f(one, 10, one, 4, one, float("inf"), None, one, None) == GSR_ERR_INVALID
    assert f(one, 10, ctypes.c_void_p(264), 4, one, 0.0, None, one, None) == GSR_ERR_INVALID and "aligned" in _err(lib)


def test_convex_hull_without_device(lib):
    pts = np.array([[x, y, z] for x in (0.0, 2.0) for y in (0.0, 2.0) for z in (-1.0, 1.0)])
    planes = np.zeros((64, 4))
    nf, bbox = ctypes.c_int64(-5), np.zeros(6)
    rc = lib.gsr_convex_hull_planes(pts.ctypes.data, 8, planes.ctypes.data, 64, ctypes.byref(nf), bbox.ctypes.data)
    assert rc == 0 and nf.value == 12 and np.array_equal(bbox, [0, 0, -1, 2, 2, 1])
    assert np.all(pts @ planes[:12, :3].T - planes[:12, 3] <= 1e-12)
    # too small a buffer: the count needed, nothing written
    small = np.full((4, 4), 7.0)
    rc = lib.gsr_convex_hull_planes(pts.ctypes.data, 8, small.ctypes.data, 4, ctypes.byref(nf), bbox.ctypes.data)
    assert rc == GSR_ERR_NOMEM and nf.value == 12 and np.all(small == 7.0)
    # degenerate: OK with 0 facets
    flat = pts.copy(); flat[:, 2] = 0.5
    rc = lib.gsr_convex_hull_planes(flat.ctypes.data, 8, planes.ctypes.data, 64, ctypes.byref(nf), bbox.ctypes.data)
    assert rc == 0 and nf.value == 0 and "degenerate" in _err(lib)
    # argument checks
    assert lib.gsr_convex_hull_planes(None, 8, planes.ctypes.data, 64, ctypes.byref(nf), bbox.ctypes.data) == GSR_ERR_INVALID
    assert lib.gsr_convex_hull_planes(pts.ctypes.data, -1, planes.ctypes.data, 64, ctypes.byref(nf), bbox.ctypes.data) == GSR_ERR_INVALID
    assert lib.gsr_convex_hull_planes(pts.ctypes.data, 8, None, 64, ctypes.byref(nf), bbox.ctypes.data) == GSR_ERR_INVALID
    assert lib.gsr_convex_hull_planes(pts.ctypes.data, 8, planes.ctypes.data, 64, None, bbox.ctypes.data) == GSR_ERR_INVALID


def test_python_hull_binding_without_device(lib):
    from diff_gaussian_rasterization import groups as G
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(3000, 3))
    h = G.convex_hull_planes(pts)
    assert not h.degenerate and h.planes.shape[1] == 4 and len(h.planes) >= 4
    ext = pts.max(0) - pts.min(0)
    assert h.tau == pytest.approx(1e-9 * np.linalg.norm(ext), rel=1e-12)
    assert np.all(pts @ h.planes[:, :3].T - h.planes[:, 3] <= 1e-9)
    assert G.convex_hull_planes(np.zeros((0, 3))).degenerate
    assert G.convex_hull_planes(pts[:3]).degenerate


def test_classifier_state_dict_layouts(tmp_path):
    from gsplat_attack.groups import load_classifier
    from gsplat_attack.objects import ObjectClassifier
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(16, 37, kernel_size=1)
    w, b = load_classifier(conv.state_dict())                   # the reference's classifier.pth layout
    assert torch.equal(w, conv.weight.detach().reshape(37, 16)) and torch.equal(b, conv.bias.detach())
    oc = ObjectClassifier(num_classes=37)
    w2, b2 = load_classifier(oc.state_dict())                   # ObjectClassifier's conv.weight / conv.bias
    assert torch.equal(w2, oc.conv.weight.detach().reshape(37, 16)) and torch.equal(b2, oc.conv.bias.detach())
    path = tmp_path / "classifier.pth"
    torch.save(conv.state_dict(), path)
    w3, b3 = load_classifier(str(path))
    assert torch.equal(w3, w) and torch.equal(b3, b)
    with pytest.raises(ValueError):
        load_classifier(torch.nn.Conv2d(16, 1025, 1).state_dict())
    with pytest.raises(ValueError):
        load_classifier(torch.nn.Conv2d(8, 4, 1).state_dict())
    with pytest.raises(KeyError):
        load_classifier({"w": torch.zeros(3, 16)})


def test_synthetic_grouping_leaves_scene_keys_alone():
    from gsplat_attack.scenes import make_scene, synthetic_grouping
    a, _, _ = make_scene("hydrant-1k", n_views=1)
    b, _, _ = make_scene("hydrant-1k", n_views=1)
    rows = torch.zeros(a._xyz.shape[0], dtype=torch.bool)
    rows[::7] = True
    sd = synthetic_grouping(a, rows, 117)
    c, _, _ = make_scene("hydrant-1k", n_views=1)
    for n in b._PARAM_ATTRS:
        assert torch.equal(getattr(b, n), getattr(c, n))        # the scene key's tensors do not depend on the helper
        if n != "_objects_dc":
            assert torch.equal(getattr(a, n), getattr(b, n))
    assert torch.equal(a._objects_dc[~rows], b._objects_dc[~rows])
    assert sd["weight"].shape == (256, 16, 1, 1) and sd["bias"].shape == (256,)
    # float64 reference of the classifier: the prototype rows are class 117, no other row is
    logits = a._objects_dc.double().reshape(-1, 16) @ sd["weight"].double().reshape(256, 16).T + sd["bias"].double()
    p = torch.softmax(logits, dim=1)[:, 117]
    assert bool((p[rows] > 0.999).all()) and bool((p[~rows] < 0.01).all())


def test_split_group_rejects_empty_selection():
    from gsplat_attack.groups import split_group
    from gsplat_attack.scenes import make_scene
    m, _, _ = make_scene("hydrant-1k", n_views=1)
    with pytest.raises(ValueError, match="no Gaussian is selected"):
        split_group(m, torch.zeros(m._xyz.shape[0], dtype=torch.bool))
    sel = torch.zeros(m._xyz.shape[0], dtype=torch.bool)
    sel[10:20] = True
    g, r = split_group(m, sel)
    assert g._xyz.shape[0] == 10 and r._xyz.shape[0] == m._xyz.shape[0] - 10
    assert torch.equal(g._features_dc, m._features_dc[sel]) and torch.equal(r._opacity, m._opacity[~sel])

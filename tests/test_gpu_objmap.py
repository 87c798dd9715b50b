"""gsr_objmap on the device against tests/objmap_cases.py: ids, stats and paint bit for bit the host build's (they share the
per-pixel source) on every case; conf, the CE terms and the gradient within the project's bound (floor 2^-22, never above
1e-3) of the float64 oracle, the margins asserted first; sentinel-filled outputs fully written and a NaN-filled workspace of
exactly the reported size without influence; the same bits from a second call, a side stream, misaligned tensors and every
subset of the optional outputs; B = 2 as two B = 1 calls; a NaN inside its own image; the user-level functions; the gradient
through the rasteriser to the model's object features; and group_bboxes against the solo render's box."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import objmap_cases as OC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
CASES = OC.cases()
BY_ID = {c.id: c for c in CASES}
OPTIONAL = ("conf", "stats", "paint", "terms", "grad")


@pytest.fixture(scope="module")
def OM():
    from diff_gaussian_rasterization import objmap_ops
    assert objmap_ops.available()
    return objmap_ops


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _off4(t):
    """A copy of t (4-byte elements) that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    k = 1 + (-(buf.data_ptr() // 4) % 4)                    # element k sits on boundary + 4
    out = buf[k:k + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def _raw(OM, x, want=OPTIONAL, stream=None, misalign=False):
    """The C call itself on sentinel-filled outputs and a NaN-filled workspace of exactly the bytes asked for.
    x: dict(objmap, weight, bias, target, palette) of numpy arrays or device tensors."""
    from diff_gaussian_rasterization._ops_common import call, workspace, workspace_bytes
    x = {k: (v if torch.is_tensor(v) else _t(v)) for k, v in x.items()}
    B, _, H, W = x["objmap"].shape
    K = x["weight"].shape[0]
    loss = "terms" in want or "grad" in want
    cs = OM.c_spec((B, H, W), K, OM.LOSS if loss else 0)
    n = workspace_bytes("gsr_objmap_workspace_bytes", cs)
    assert (n > 0) == loss
    ws = workspace(n, DEV)
    ws.view(torch.float32).fill_(float("nan"))
    shift = _off4 if misalign else (lambda t: t)
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=DEV)
    out = dict(ids=shift(full((B, H, W), -7, torch.int32)),
               conf=shift(full((B, H, W), SENTINEL, torch.float32)) if "conf" in want else None,
               stats=shift(full((B, K, 5), -7, torch.int32)) if "stats" in want else None,
               paint=full((B, H, W, 3), 7, torch.uint8) if "paint" in want else None,
               terms=shift(full((B, 2), SENTINEL, torch.float32)) if "terms" in want else None,
               grad=shift(full((B, OC.CH, H, W), SENTINEL, torch.float32)) if "grad" in want else None)
    if misalign:
        x = {k: (shift(v) if v.element_size() == 4 else v) for k, v in x.items()}
    ptr = lambda t: t.data_ptr() if t is not None else None
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(DEV)):
        call("gsr_objmap", torch.device(DEV), ctypes.byref(cs), x["objmap"].data_ptr(), x["weight"].data_ptr(), x["bias"].data_ptr(),
             x["target"].data_ptr() if loss else None, x["palette"].data_ptr() if "paint" in want else None,
             ws.data_ptr() if n else None, n, *(ptr(out[k]) for k in ("ids",) + OPTIONAL))
    torch.cuda.synchronize()
    return out


def _same(a, b, keys):
    for k in keys:
        assert _bits(a[k]) == _bits(b[k]), k


# ---- 1. the host build and the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_device_matches_the_host_bits_and_the_oracle(OM, c):
    assert OC.margins_ok(c)
    got, host = _raw(OM, OC.inputs(c)), OC.host_run(c)
    assert not (got["ids"] == -7).any() and not (got["stats"] == -7).any()      # every element written
    for k in ("conf", "terms", "grad"):
        assert not (got[k] == SENTINEL).any(), k
    for k in ("ids", "stats", "paint"):
        assert _bits(got[k]) == host[k].tobytes(), k
    assert _bits(got["terms"][:, 1]) == host["terms"][:, 1].tobytes()           # the counted pixels
    fails = OC.check(got, c, f"device {c.id}")
    assert not fails, fails


# ---- 2. what must not matter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("random-2x17x33x5", "nonfinite-2x9x31x256", "exact-1x3x3x1024"))
def test_repeat_stream_alignment_and_every_subset_of_outputs(OM, name):
    x = OC.inputs(BY_ID[name])
    base = _raw(OM, x)
    keys = ("ids",) + OPTIONAL
    _same(_raw(OM, x), base, keys)                                                # a second call
    _same(_raw(OM, x, stream=torch.cuda.Stream(device=DEV)), base, keys)          # a side stream
    _same(_raw(OM, x, misalign=True), base, keys)                                 # 4 bytes past a 16-byte boundary
    for r in range(len(OPTIONAL)):
        for want in itertools.combinations(OPTIONAL, r):
            got = _raw(OM, x, want=want)
            _same(got, base, ("ids",) + want)
            assert all(got[k] is None for k in OPTIONAL if k not in want)
    # the binding: outputs from torch.empty, the cached workspace -- and again
    for _ in range(2):
        out = OM.objmap_forward(_t(x["objmap"]), _t(x["weight"]), _t(x["bias"]), target=_t(x["target"]), palette=_t(x["palette"]),
                                want_conf=True, want_stats=True, want_paint=True, want_grad=True)
        _same(out._asdict(), base, keys)
    plain = OM.objmap_forward(_t(x["objmap"]), _t(x["weight"]), _t(x["bias"]))
    assert _bits(plain.ids) == _bits(base["ids"]) and all(v is None for v in plain[1:])


@pytest.mark.parametrize("name", ("random-2x17x33x5", "nonfinite-2x17x33x5", "random-2x9x31x256"))
def test_a_batch_is_its_images_and_a_nan_stays_in_its_own(OM, name):
    c = BY_ID[name]
    x = OC.inputs(c)
    both = _raw(OM, x)
    for b in range(2):
        one = _raw(OM, dict(x, objmap=x["objmap"][b:b + 1], target=x["target"][b:b + 1]))
        for k in ("ids",) + OPTIONAL:
            assert _bits(both[k][b]) == _bits(one[k][0]), (k, b)
    if c.kind == "nonfinite":
        assert torch.isnan(both["terms"][0, 0]) and torch.isnan(both["grad"][0]).any()
        assert torch.isfinite(both["terms"][1]).all() and torch.isfinite(both["grad"][1]).all() and torch.isfinite(both["conf"][1]).all()


# ---- 3. the user-level functions ---------------------------------------------------------------------------------------------------
def _getbbox(mask):
    try:
        from PIL import Image
        return Image.fromarray(mask.astype(np.uint8) * 255).getbbox()
    except ImportError:                                                           # the same convention in numpy
        ys, xs = np.nonzero(mask)
        return (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if len(ys) else None


def test_segment_objects_and_object_boxes(OM):
    from gsplat_attack import objects as GO
    c = BY_ID["exact-2x17x33x5"]
    x, host = OC.inputs(c), OC.host_run(c)
    clf = GO.ObjectClassifier(num_classes=5)
    with torch.no_grad():
        clf.conv.weight.copy_(torch.from_numpy(np.array(x["weight"])).view(5, 16, 1, 1))
        clf.conv.bias.copy_(torch.from_numpy(np.array(x["bias"])))
    maps = GO.segment_objects(_t(x["objmap"]), clf.to(DEV), conf=True, paint=True)
    assert maps.ids.dtype == torch.int32 and tuple(maps.paint.shape) == (2, 17, 33, 3) and maps.paint.dtype == torch.uint8
    for k in ("ids", "stats", "paint"):
        assert _bits(getattr(maps, k)) == host[k].tobytes(), k
    assert torch.equal(maps.conf, _raw(OM, x, want=("conf",))["conf"])
    clf = clf.cpu()
    for b in range(2):                                                            # the torch expression, map by map
        want = GO.predict_objects(torch.from_numpy(np.array(x["objmap"][b])), clf)
        one = GO.segment_objects(_t(x["objmap"][b]), (clf.conv.weight, clf.conv.bias))
        assert one.ids.shape == want.shape and torch.equal(one.ids.cpu().long(), want)
        assert torch.equal(one.stats, maps.stats[b]) and one.conf is None and one.paint is None
        assert np.array_equal(maps.paint[b].cpu().numpy(), GO.visualize_obj(want.numpy()))
    ids = host["ids"]
    present = [int(k) for k in np.unique(ids[0])]
    sel = present[:2] if len(present) >= 2 else [present[0], (present[0] + 1) % 5]
    boxes = GO.object_boxes(maps.stats, sel)
    for b in range(2):
        mask = np.isin(ids[b], sel)
        assert boxes[b] == (_getbbox(mask), int(mask.sum())), b
    assert GO.object_boxes(maps.stats[1], sel) == boxes[1]


def test_object_ce_reaches_the_object_features(OM):
    from gsplat_attack import objects as GO
    from gsplat_attack.renderer import PipelineParams, render
    from gsplat_attack.scenes import make_scene
    model, cams, _ = make_scene("hydrant-1k", device=torch.device(DEV), P=200, width=64, height=64, n_views=1)
    bg = torch.zeros(3, device=DEV)
    g = torch.Generator().manual_seed(3)
    wt, bs = (torch.randn(5, 16, generator=g) * 0.5).to(DEV), (torch.randn(5, generator=g) * 0.1).to(DEV)
    target = torch.randint(-1, 6, (64, 64), generator=g).to(DEV)                  # -1 and 5: ignored

    om = render(cams[0], model, PipelineParams(), bg)["render_object"]
    assert om.requires_grad and tuple(om.shape) == (16, 64, 64)
    loss = GO.object_ce(om, target, (wt, bs))
    assert tuple(loss.shape) == (1,) and loss.requires_grad and torch.isfinite(loss).all() and loss.item() > 0
    loss.sum().backward()
    got = model._objects_dc.grad.detach().clone()
    assert torch.isfinite(got).all() and got.abs().max() > 0

    model.zero_grad()                                                             # ... and by hand through the rasteriser
    om2 = render(cams[0], model, PipelineParams(), bg)["render_object"]
    raw = OM.objmap_forward(om2.detach(), wt, bs, target=target, want_grad=True)
    assert _bits(raw.terms[:, 0]) == _bits(loss) and raw.terms[0, 1] == ((target >= 0) & (target < 5)).sum()
    om2.backward(raw.grad[0])
    assert torch.equal(model._objects_dc.grad, got)

    model.zero_grad()                                                             # an upstream factor scales it
    om3 = render(cams[0], model, PipelineParams(), bg)["render_object"].unsqueeze(0)
    (GO.object_ce(om3, target.unsqueeze(0), (wt, bs)) * 0.0).sum().backward()
    assert not model._objects_dc.grad.any()
    with torch.no_grad():
        assert _bits(GO.object_ce(om2.detach(), target, (wt, bs))) == _bits(loss)
    with pytest.raises(ValueError, match="must not require grad"):
        OM.object_ce(om2.detach(), wt.clone().requires_grad_(True), bs, target)      # (the user level detaches a module's parameters)


def test_group_bboxes_inside_the_solo_box():
    from gsplat_attack import objects as GO
    from gsplat_attack.attack import benign_bboxes
    from gsplat_attack.renderer import PipelineParams, render
    full, solos, cam, clf = OC.two_object_scene(torch.device(DEV))
    black = torch.zeros(3, device=DEV)
    pipe = PipelineParams(skip_objects=True, aux_outputs=True)
    with torch.no_grad():
        a1, a2 = (render(cam, m, pipe, black)["render_alpha"][0] > OC.SOLO_ALPHA for m in solos)
    hidden = int((a1 & a2).sum()) / int(a1.sum())
    print(f"object 2 covers {hidden:.3f} of object 1's {int(a1.sum())} pixels")
    assert int(a1.sum()) > 100 and 0 < hidden < 0.5                              # the scene: occluded, but less than half
    solo = benign_bboxes(solos[0], [cam], alpha_threshold=OC.SOLO_ALPHA)[0]
    box, = GO.group_bboxes(full, [cam], clf, [1])
    scene = render(cam, full, PipelineParams(), black)["render_object"].detach()
    again, count = GO.object_boxes(GO.segment_objects(scene, clf).stats, [1])
    assert again == box                                                          # ... is object_boxes of the full render
    print(f"in the scene {box} ({count} pixels), alone {solo}")
    assert box is not None and 0 < count < int(a1.sum())
    assert solo[0] <= box[0] and solo[1] <= box[1] and box[2] <= solo[2] and box[3] <= solo[3]
    area = lambda r: (r[2] - r[0]) * (r[3] - r[1])
    assert area(box) / area(solo) > 0.5                                          # box inside solo: that ratio is the IoU
    assert GO.group_bboxes(full, [cam], clf, [0, 1, 2]) == [(0, 0, OC.SCENE_SIZE, OC.SCENE_SIZE)]

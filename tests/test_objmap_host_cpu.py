"""The object-map classifier's scalar source (csrc/gsr_objmap.h) built for the host, against tests/objmap_cases.py: ids equal
the float64 oracle's wherever its decision is safe from float32 rounding (everywhere on the exact kind, ties included); conf,
the CE terms and the gradient within the project's bound; the oracle's own gradient against central finite differences;
stats against a numpy recount; paint against visualize_obj; and terms that do not depend on the other outputs asked for.
Needs no GPU."""
import numpy as np
import pytest
import torch

import objmap_cases as OC

CASES = OC.cases()
BY_ID = {c.id: c for c in CASES}


def test_limits_match_the_binding():
    from diff_gaussian_rasterization import objmap_ops as OM
    assert OC.host_limits() == [OM.CHANNELS, OM.MAX_CLASSES, 256, OM.LOSS] == [16, 1024, 256, 1]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_host_matches_the_oracle(c):
    assert OC.margins_ok(c)
    host = OC.host_run(c)
    for k, v in host.items():
        assert not (v == (7 if k == "paint" else -7)).all(), k                      # written
    fails = OC.check(host, c, f"host {c.id}")
    assert not fails, fails
    ref = OC.reference(c)
    if c.kind == "exact":
        assert not ref["fragile"].any() and np.array_equal(host["ids"], ref["o64"]["ids"])
        x = OC.inputs(c)
        dup = [k for k in range(1, c.shape[3]) if any((x["weight"][k] == x["weight"][j]).all() and x["bias"][k] == x["bias"][j] for j in range(k))]
        assert not np.isin(host["ids"], dup).any()                                  # of two equal rows the lower class wins
    assert host["terms"][:, 1].tolist() == ref["o64"]["terms"][:, 1].tolist()       # the counted pixels, exactly
    if c.shape in OC.ALL_IGNORED:
        b = OC.ALL_IGNORED[c.shape]
        assert host["terms"][b].tolist() == [0.0, 0.0] and not host["grad"][b].any()


@pytest.mark.parametrize("c", [c for c in CASES if c.kind in ("nonfinite", "nanrow")], ids=lambda c: c.id)
def test_non_finite_inputs(c):
    x, host, K = OC.inputs(c), OC.host_run(c), c.shape[3]
    B, H, W, _ = c.shape
    if c.kind == "nanrow":
        assert not (host["ids"] == K // 2).any() and (host["ids"] >= 0).all()       # that class never wins
        clean = np.delete(x["weight"], K // 2, axis=0), np.delete(x["bias"], K // 2)
        other = OC.host_arrays(x["objmap"], *clean, terms=False, grad=False, paint=False, conf=False)["ids"]
        assert np.array_equal(np.where(host["ids"] > K // 2, host["ids"] - 1, host["ids"]), other)   # the others are unaffected
        assert np.isnan(host["conf"]).all() and np.isnan(host["terms"][0, 0])       # ... but it reaches every softmax sum
        return
    assert host["ids"][0, H // 2, W // 2] == -1 and host["conf"][0, H // 2, W // 2] == 0             # every logit NaN
    assert not host["grad"][0, :, H // 2, W // 2].any()
    assert host["ids"][0, H - 1, W - 1] == 1 and np.isnan(host["conf"][0, H - 1, W - 1])             # class 0: inf - inf; class 1: +inf
    one = OC.host_arrays(x["objmap"][1:], x["weight"], x["bias"], x["target"][1:], x["palette"])
    for k in ("ids", "conf", "stats", "paint", "terms", "grad"):                    # a NaN stays inside its own image
        assert host[k][1].tobytes() == one[k][0].tobytes(), k
    assert np.isfinite(host["conf"][1]).all() and np.isfinite(host["grad"][1]).all()


def test_oracle_gradient_against_central_differences():
    c = BY_ID["random-1x7x5x2"]
    x = OC.inputs(c)
    f = x["objmap"].astype(np.float64)
    loss = lambda a: OC.run_arrays(a, x["weight"], x["bias"], x["target"], torch.float64)["terms"][:, 0].sum()
    g = OC.reference(c)["o64"]["grad"]
    h, worst = 1e-6, 0.0
    for idx in np.ndindex(*f.shape):
        up, dn = f.copy(), f.copy()
        up[idx] += h
        dn[idx] -= h
        worst = max(worst, abs((loss(up) - loss(dn)) / (2 * h) - g[idx]))
    print(f"central differences: worst {worst:.3e} of max |g| {np.abs(g).max():.3e}")
    assert np.abs(g).max() > 1e-4 and worst <= 1e-8                                # O(h^2) truncation + 1e-16 / h rounding


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_stats_and_paint(c):
    from gsplat_attack.objects import id2rgb, visualize_obj
    host, K = OC.host_run(c), c.shape[3]
    want = OC.recount(host["ids"], K)
    assert host["stats"].tobytes() == want.tobytes()
    absent = want[:, :, 0] == 0
    assert not host["stats"][absent].any() and int(want[:, :, 0].sum()) == int((host["ids"] >= 0).sum())
    for b in range(c.shape[0]):
        ids, on = host["ids"][b], host["ids"][b] >= 0
        assert not host["paint"][b][~on].any()                                      # id -1: black
        if ids.max() <= 256:
            assert np.array_equal(host["paint"][b][on], visualize_obj(np.where(on, ids, 0))[on])
        else:                                                                       # visualize_obj refuses ids above 256
            assert np.array_equal(host["paint"][b][on], np.stack([id2rgb(int(i), K) for i in ids[on]]))


@pytest.mark.parametrize("name", ["random-2x17x33x5", "nonfinite-2x17x33x5", "exact-1x3x3x1024"])
def test_outputs_do_not_depend_on_each_other(name):
    c = BY_ID[name]
    x, full = OC.inputs(c), OC.host_run(c)
    for mask in range(32):
        kw = dict(conf=bool(mask & 1), stats=bool(mask & 2), paint=bool(mask & 4), terms=bool(mask & 8), grad=bool(mask & 16))
        got = OC.host_arrays(x["objmap"], x["weight"], x["bias"], x["target"], x["palette"], **kw)
        assert got["ids"].tobytes() == full["ids"].tobytes(), kw
        for k, on in kw.items():
            assert (got[k] is None) == (not on) and (not on or got[k].tobytes() == full[k].tobytes()), (k, kw)

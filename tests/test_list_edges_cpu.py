"""Preconditions of tests/test_gpu_list_edges.py, from oracle-R alone: on every scene of tests/list_edge_scenes.py the
designed list lengths and stop indices are the oracle's, NO pixel and NO Gaussian is fragile (the cap is zero: a scene that
cannot meet it gets other parameters), no depth near-tie exists, and oracle-R run in float32 stays inside every threshold
the GPU test applies -- so those thresholds are ones a correct float32 implementation can meet."""
import numpy as np
import pytest
import torch

import list_edge_scenes as S
from oracle import oracle_r as O
from util import grad_error

RGB_TOL, OBJ_TOL, GRAD_TOL = 1e-4, 3e-4, 1e-3      # README parity bound; smoke()'s object bound; the project's gradient bound

CASES = [(k, 0) for k in S.SINGLE_VIEW] + [(("D", 16), v) for v in range(16)]


def _id(c):
    return f"{c[0] if isinstance(c[0], str) else 'D'}-v{c[1]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_designed_facts_are_the_oracles_and_nothing_is_fragile(case):
    key, view = case
    sc = S.get(key)
    f = sc.facts[view]
    r = S.oracle_run(sc, view)
    a = S.activate({k: v.double() for k, v in sc.raw.items()})
    st = S.settings(sc.cams[view], torch.tensor(S.BG), O.Settings)
    g = O.preprocess(a["means3D"], a["scales"], a["rotations"], None, st)
    gid, ranges, _ = O.build_tile_lists(g, sc.H, sc.W)
    lens = (ranges[:, 1] - ranges[:, 0]).view(f.tile_len.shape).numpy()
    assert np.array_equal(lens, f.tile_len), "list lengths"
    assert r.num_rendered == int(f.tile_len.sum())
    # the default footprint cull drops no pair of these scenes: lengths and list positions are the oracle's under it too
    assert np.array_equal(f.tile_len_cull, f.tile_len) and np.array_equal(f.n_contrib_cull, f.n_contrib)
    assert np.array_equal(r.n_contrib.numpy(), f.n_contrib), "stop indices"
    assert np.abs(r.final_T.numpy() - f.final_T).max() < 1e-3      # (the model leaves out nothing that matters)
    assert r.fragile_px == 0 and r.fragile_gauss == 0, (r.fragile_px, r.fragile_gauss)
    z, ez = g.depth.double(), g.e_depth.double()
    for t in range(ranges.shape[0]):
        ids = gid[int(ranges[t, 0]):int(ranges[t, 1])]
        if ids.numel() > 1:
            assert bool(((z[ids][1:] - z[ids][:-1]) > 100.0 * (ez[ids][1:] + ez[ids][:-1])).all()), f"tile {t}: depth near-tie"
    if view == 0 and hasattr(sc, "designed_len"):
        for (tx, ty), n in sc.designed_len.items():
            assert lens[ty, tx] == n
    dead = S.dead_gaussians(sc) if len(sc.facts) == 1 else ~f.blended
    if hasattr(sc, "stops") and getattr(sc, "tiny", True):
        # every designed stop index > 40 has its stopping entry (and the seven behind it) among the never-blended ones, and
        # that entry lies right behind pixel (8, 8)'s n_contrib: the exact-zero check bites on an off-by-one there
        ids = S.stopper_ids(sc)
        assert len(ids) == S.STOPPERS * sum(s_ > S.KILL for s_ in sc.stops.values()) > 0 and S.dead_gaussians(sc)[ids].all()
        if view == 0:
            for (tx, ty), s_ in sc.stops.items():
                assert r.n_contrib[16 * ty + 8, 16 * tx + 8] == s_
                if s_ > S.KILL:
                    nxt = (sc.tile[:, 0] == tx) & (sc.tile[:, 1] == ty) & (sc.pos == s_ + 1)
                    assert nxt.sum() == 1 and dead[nxt].all(), f"stop {s_}: the stopping entry is blended by some pixel"
    for c in "CODA":
        for k in S.RAW:
            assert float(r.grads[c][k][torch.tensor(dead)].abs().max() if dead.any() else 0.0) == 0.0, (c, k)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_float32_oracle_stays_inside_every_threshold(case):
    key, view = case
    sc = S.get(key)
    r64, r32 = S.oracle_run(sc, view), S.oracle_run(sc, view, torch.float32)
    assert torch.equal(r32.n_contrib, r64.n_contrib) and torch.equal(r32.radii, r64.radii)
    e = lambda x, y: (x.double() - y).abs().max().item() if x.numel() else 0.0
    eC, eT, eO = e(r32.color, r64.color), e(r32.final_T, r64.final_T), e(r32.objects, r64.objects)
    eA, eD = e(r32.alpha, r64.alpha), e(r32.depth, r64.depth) / r64.z_far
    print(f"[{sc.name} v{view}] f32 oracle: colour {eC:.2e} final_T {eT:.2e} objects {eO:.2e} alpha {eA:.2e} depth/z_far {eD:.2e}")
    assert eC <= RGB_TOL and eT <= RGB_TOL and eA <= RGB_TOL and eD <= RGB_TOL and eO <= OBJ_TOL
    for terms in ("C", "CO", "CA", "CDA"):
        for k in S.RAW + S.CLASSIC + ("means2D",):
            norm, _ = grad_error(S.grad_sum(r32, terms, k), S.grad_sum(r64, terms, k))
            assert norm <= GRAD_TOL, (terms, k, norm)

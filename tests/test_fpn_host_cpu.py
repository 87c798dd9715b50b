"""The FPN RoI pooler's scalar source on the host (tests/host_math/fpn_host.cpp over csrc/gsr_fpn.h and csrc/gsr_rcnn.h)
against the oracle of tests/fpn_cases.py: levels, lists and counts integer-equal, in float32 and in float64; pooled values
and every level's gradient within the project's bound of the float64 oracle; and a float32 restatement of Detectron2's
log2 formula agreeing on every finite row of non-negative area.  Needs no GPU."""
import numpy as np
import pytest

import fpn_cases as FC


@pytest.fixture(scope="module")
def host():
    return FC.host_lib()


def test_every_row_is_declared_and_the_table_holds():
    assert FC.check_declarations()
    assert FC.THR == (0.0, 0.5, 1.0, 2.0)


@pytest.mark.parametrize("n_roi", (FC.N_ROI, FC.N_ROI_ZERO, None), ids=("counts", "count-0", "no-counts"))
def test_host_levels_lists_and_counts_equal_the_oracle(host, n_roi):
    lv, lists, counts = FC.oracle_levels(FC.ROIS, n_roi, 2)
    h = FC.host_assign(host, n_roi=n_roi)
    assert np.array_equal(h["roi_level"], lv) and np.array_equal(h["roi_level64"], lv)
    assert np.array_equal(h["level_count"], counts) and FC.lists_equal(h["level_list"], h["level_count"], lists)
    for b in range(FC.B):
        for l in range(FC.NL):
            n = int(counts[b, l])
            assert (h["level_list"][b, l, n:] == FC.ISENT).all()                      # nothing beyond the live prefix
            assert sorted(lists[b][l]) == lists[b][l]
    if n_roi is FC.N_ROI_ZERO:
        assert (lv[1] == -1).all() and (counts[1] == 0).all()


def test_float32_oracle_and_detectron2_formula_agree():
    lv64, _, _ = FC.oracle_levels(FC.ROIS, None, 1)
    lv32, _, _ = FC.oracle_levels(FC.ROIS, None, 1, dtype=np.float32)
    assert np.array_equal(lv64, lv32)
    d2 = FC.detectron2_levels_f32(FC.ROIS)
    q = FC.level_q(FC.ROIS)
    ok = np.isfinite(FC.ROIS).all(-1) & ~np.isnan(q)                                  # finite rows of non-negative area
    assert ok.sum() >= 30 and np.array_equal(d2[ok], lv64[ok])


def test_one_level_and_five_levels(host):
    one = FC.c_spec(sizes=FC.SIZES[:1], strides=FC.STRIDES[:1], thr=(0.0,))
    h = FC.host_assign(host, spec=one)
    lv, lists, counts = FC.oracle_levels(FC.ROIS, FC.N_ROI, 2, thr=(0.0,))
    assert np.array_equal(h["roi_level"], lv) and set(np.unique(lv)) == {-1, 0} and FC.lists_equal(h["level_list"], h["level_count"], lists)
    thr5 = (0.0, 0.25, 0.5, 1.0, 2.0)
    five = FC.c_spec(sizes=((194, 250),) + FC.SIZES, strides=(2,) + FC.STRIDES, thr=thr5)
    h = FC.host_assign(host, spec=five)
    lv, lists, counts = FC.oracle_levels(FC.ROIS, FC.N_ROI, 2, thr=thr5)
    assert np.array_equal(h["roi_level"], lv) and lv.max() == 4 and FC.lists_equal(h["level_list"], h["level_count"], lists)


@pytest.mark.parametrize("c", FC.CASES, ids=lambda c: c.id)
def test_host_pooled_and_gradients_match_the_oracle(host, c):
    ref = FC.reference(c)
    assert FC.margins_ok(ref), ref["gap_grid"]
    got = FC.host_pool(host, c)
    fails = []
    for k in FC.COMPARED:
        e, y = FC.err(got[k], ref["o64"][k]), ref["yard"][k]
        print(f"host {c.id} {k}: err {e:.3e} yardstick {y:.3e} bound {FC.bound(y):.3e}")
        if not e <= FC.bound(y):
            fails.append((k, e, FC.bound(y)))
    assert not fails, fails
    lv, _, _ = FC.oracle_levels(FC.ROIS, FC.N_ROI, 2)
    assert (got["pooled"][lv == -1] == 0).all()
    assert (got[f"grad{FC.NL - 1}"][1] == 0).all()                                    # image 1 has no RoI of the last level
    b, s = FC.INVERTED                                                                # the inverted RoI: level 0, backwards or grid 0
    assert FC.ROIS[b, s, 2] < FC.ROIS[b, s, 0] and lv[b, s] == 0
    for p in (ref["o64"]["pooled"][b, s].numpy(), got["pooled"][b, s]):
        assert (float(np.abs(p).max()) > 0) == (c.ratio > 0)
    assert (ref["o64"]["grids"][0, b, s].min() == 0) == (c.ratio == 0)


def test_host_exact_edges_by_hand(host):
    """The samples exactly at -1 and at n (valid: the border cell with weight 1) and the next positions further out (0), through
    the pooler's host build on a one-level pyramid of stride 1: the values rcnn_cases.roi_edge_inputs writes out by hand."""
    _, _, _, pooled, gf = FC.edge_inputs()
    got_p, got_g = FC.host_pool_edges(host)
    assert np.array_equal(got_p[0, :, :, 0, 0], pooled) and np.array_equal(got_g[0], gf)

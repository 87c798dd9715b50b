"""The detection metrics' scalar source (csrc/gsr_deteval.h) on the CPU: tests/host_math/deteval_host.cpp runs it in plain loops over
the header the kernels compile.  Held to the float64 oracle of tests/deteval_cases.py on every case -- integers equal, doubles
bit for bit -- plus the hand-derived literal and what each case is there to show.  No GPU."""
import ctypes

import numpy as np
import pytest

import deteval_cases as DC


@pytest.mark.parametrize("name", DC.ALL)
def test_host_build_matches_oracle(name):
    spec, batches = DC.case(name)
    DC.check(f"host {name}", DC.host_run(spec, batches), DC.oracle(name))


def test_literal():
    """rc = [1/3, 1/3, 2/3], envelope [1, 2/3, 2/3]: precision 1 for 34 thresholds, 2/3 for 33, 0 for 34; AP = 56/101, AR = 2/3"""
    spec, batches = DC.literal()
    for got in (DC.host_run(spec, batches), DC.oracle_run(spec, batches)):
        assert got["dt_match"][0, 0, 0].tolist() == [0, -1, 1] and got["npig"].tolist() == [[3]]
        p = got["precision"][0, :, 0, 0, 0]
        one = 1 / (1 + DC.EPS)                                    # COCOeval's precision of a lone true positive: the double below 1
        assert one < 1.0 and (p[:34] == one).all() and DC.same(p[34:67], np.full(33, 2 / (3 + DC.EPS))) and (p[67:] == 0.0).all()
        assert DC.same(got["scores"][0, :, 0, 0, 0], np.r_[np.full(34, np.float32(0.9)), np.full(33, np.float32(0.7)), np.zeros(34)].astype(np.float64))
        assert got["recall"][0, 0, 0, 0] == 2 / 3
        st = got["stats"]
        assert abs(st[0] - 56 / 101) <= 101 * 2.0 ** -52 and abs(st[1] - 56 / 101) <= 101 * 2.0 ** -52 and st[2] == -1.0
        assert (st[3:6] == -1).all() and st[6] == 2 / 3 and st[7] == st[8] == -1 and (st[9:12] == -1).all()
        assert st[12] == st[0] and st[13] == st[6]


def test_counts_clamp_and_dead_positions():
    spec, batches = DC.case("counts-D129")
    got = DC.host_run(spec, batches)
    live = (got["dt_order"] >= 0).sum(1).tolist()
    assert live == [0, 1, 63, 64, 65, 129, 129, 0]              # every row of these images is live: the count, clamped to 0..D
    for b, n in enumerate(live):
        assert (got["dt_match"][b, :, :, n:] == -1).all() and (got["dt_ignore"][b, :, :, n:] == 0).all() and (got["dt_rank"][b, n:] == -1).all()
        s = batches[0][0][b, got["dt_order"][b, :n], 4]
        assert (np.diff(s) <= 0).all()
        ties = np.diff(s) == 0
        assert (np.diff(got["dt_order"][b, :n])[ties] > 0).all() and (n < 10 or ties.any())     # equal scores keep row order


def test_ties_across_images_and_signed_zero():
    spec, batches = DC.case("ties")
    got = DC.host_run(spec, batches)
    assert (got["dt_order"][2] >= 0).sum() == 31
    o = got["dt_order"][2, :31]
    zeros = [int(r) for r in o if r < 4]
    assert zeros == [0, 1, 2, 3]                                # -0 and +0 are one score: row order decides
    assert np.array_equal(got["dt_order"][0], got["dt_order"][1])            # two images of the same detections
    assert DC.host_lib().deh_score_key(ctypes.c_float(-0.0)) == DC.host_lib().deh_score_key(ctypes.c_float(0.0))
    keys = [DC.host_lib().deh_score_key(ctypes.c_float(v)) for v in (np.inf, 1.0, 1e-30, 0.0, -1e-30, -1.0, -np.inf)]
    assert keys == sorted(keys) and len(set(keys)) == 7


def test_dead_rows_take_no_part():
    spec, batches = DC.case("dead-rows")
    got = DC.host_run(spec, batches)
    assert got["dt_order"][0].tolist() == [5, 6, -1, -1, -1, -1, -1, -1]     # NaN score, NaN coordinate, 2.5, K, -1 and row 7 are dead
    assert got["gt_ignore"][0, 0].tolist() == [0, 2, 2, 2, 0]               # a NaN box, class K and class -1
    assert got["npig"][:, 0].tolist() == [1, 1, 0]
    assert got["dt_match"][0, 0, 0, :2].tolist() == [0, 4]


def test_iou_exactly_at_the_threshold():
    spec, batches = DC.case("iou-at-threshold")
    lib = DC.host_lib()

    def iou(a, b):
        a, b = np.array(a, np.float32), np.array(b, np.float32)
        return lib.deh_iou(a.ctypes.data, b.ctypes.data)
    assert iou((0, 0, 1, 1), (0, 0, 2, 1)) == 0.5 and iou((5, 5, 9, 9), (5, 5, 9, 9)) == 1.0
    assert 1 - 1e-5 < iou((20, 20, 21, 21), (20, 20, 21, 21.000002)) < 1 - 1e-10
    assert iou((0, 0, np.inf, 1), (0, 0, np.inf, 1)) == 0.0                  # inf / inf: a NaN IoU counts as 0
    got = DC.host_run(spec, batches)
    assert got["dt_match"][0, 0, 0, :3].tolist() == [0, 1, 2]               # at 0.5: exactly 0.5 matches
    assert got["dt_match"][0, 0, 1, :3].tolist() == [-1, 1, -1]             # at 1.0 (held to 1 - 1e-10): exactly 1 matches, 1 - 2e-6 not


def test_equal_iou_takes_the_later_row():
    got = DC.host_run(*DC.case("equal-iou"))
    assert got["dt_match"][0, 0, 0].tolist() == [2, 1] and got["gt_match"][0, 0, 0].tolist() == [-1, 1, 0]


def test_ignored_row_rules():
    got = DC.host_run(*DC.case("ignore-rules"))
    assert got["gt_ignore"][0].tolist() == [[0, 0], [1, 0], [0, 1]]
    # image 0, range 1: at 0.5 the counted row (IoU 0.6) is taken and the walk stops in front of the ignored row of IoU 0.91; the
    # second detection then takes the ignored row.  At 0.75 only the ignored row qualifies.
    assert got["dt_match"][0, 1, 0, :2].tolist() == [1, 0] and got["dt_ignore"][0, 1, 0, :2].tolist() == [0, 1]
    assert got["dt_match"][0, 1, 1, :2].tolist() == [0, -1] and got["dt_ignore"][0, 1, 1, :2].tolist() == [1, 1]
    assert got["dt_match"][0, 0, 0, :2].tolist() == [0, 1]                  # all areas: the best IoU
    assert got["dt_match"][1, 1, 0, 0] == 0 and got["dt_ignore"][1, 1, 0, 0] == 1
    # image 2: unmatched detections of area 25, 400 and 8100 under 100..500 and under 500..
    assert got["dt_ignore"][2, 1, 0].tolist() == [1, 0, 1] and got["dt_ignore"][2, 2, 0].tolist() == [1, 1, 0] and got["dt_ignore"][2, 0, 0].tolist() == [0, 0, 0]


def test_caps_count_ranks_within_image_and_class():
    spec, batches = DC.case("caps")
    got = DC.host_run(spec, batches)
    cls = batches[0][0][0, got["dt_order"][0], 5]
    assert sorted(got["dt_rank"][0][cls == 1].tolist()) == list(range(12)) and (cls == 1).sum() == 12
    ref = DC.oracle("caps")
    r = ref["recall"][0, 1, 0]                                   # class 1: more detections admitted, never less recall
    assert r[0] <= r[1] <= r[2] and r[0] < r[2]


def test_empty_classes():
    got = DC.host_run(*DC.case("empty-classes"))
    assert got["npig"][:, 0].tolist()[1] == 0 and got["npig"][2, 0] > 0 and got["npig"][3, 0] == 0
    assert (got["precision"][:, :, 1] == -1).all() and (got["recall"][:, 1] == -1).all() and (got["scores"][:, :, 3] == -1).all()
    assert (got["precision"][:, :, 2, 0] == 0).all() and (got["recall"][:, 2, 0] == 0).all()     # gt, no detections
    only0 = got["precision"][:, :, [0, 2], 0, -1]
    assert got["stats"][0] == pytest.approx(only0.mean(), abs=only0.size * 2.0 ** -52)          # classes 1 and 3 stay out of the mean


def test_recall_thresholds_are_the_callers():
    spec, batches = DC.case("recall-100")
    lin, div = np.linspace(0.0, 1.0, 101), np.arange(101) / 100.0
    differ = np.flatnonzero(lin != div)
    assert len(differ) > 0
    refs = []
    for rec in (lin, div):
        ref = DC.oracle_run(spec, batches, rec)
        DC.check("host recall-100", DC.host_run(spec, batches, rec), ref)
        refs.append(ref)
    assert refs[0]["npig"].tolist() == [[100]]
    assert not DC.same(refs[0]["precision"], refs[1]["precision"])           # tp / 100 lands between the two values of some threshold


def test_scan_carry_segments_straddle_the_step():
    spec, batches = DC.case("scan-carry")
    ch = DC.limits()["ACC_CHUNK"]
    ref = DC.oracle("scan-carry")
    cls = np.concatenate([b[0] for b in batches])[..., 5].reshape(-1)
    assert [int((cls == k).sum()) for k in range(spec.K)] == [ch - 1, ch, ch + 1, 2 * ch + 1, 1]
    assert (ref["npig"][:, 0] > 0).all()


def test_summary_against_numpy_mean():
    for name in ("T10-batches", "caps", "ignore-rules", "T1"):
        spec, _ = DC.case(name)
        ref = DC.oracle(name)
        for i, sl in enumerate(DC.stat_slices(spec, ref["precision"], ref["recall"])):
            v = np.zeros(0) if sl is None else sl[sl > -1]
            assert abs(ref["stats"][i] - (np.mean(v) if v.size else -1.0)) <= max(v.size, 1) * 2.0 ** -52, (name, i)


def test_host_refusals():
    lib = DC.host_lib()
    spec, batches = DC.case("literal")
    for bad in (dict(K=0), dict(K=65536), dict(D=0), dict(D=4097), dict(M=-1), dict(M=257), dict(max_dets=(0,)), dict(max_dets=(4,)),
                dict(max_dets=(2, 1)), dict(iou_thrs=[DC.NAN]), dict(areas=((0, DC.NAN),))):
        cs = DC.c_spec(spec.replace(**bad))
        assert lib.deh_summarize(ctypes.byref(cs), 8, 8, 8) == 1, bad

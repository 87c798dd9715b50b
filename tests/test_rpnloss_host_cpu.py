"""The RPN loss stage's scalar source on the host (tests/host_math/rpnloss_host.cpp over csrc/gsr_rpnloss.h) against the
oracle of tests/rpnloss_cases.py: pre-labels, labels, matched rows and counts integer-equal on every case, the sample equal to
sorted() on (key, r), loss and both gradients within the project's bound of the float64 oracle in float and in double, and
the designed rows doing what they were designed for.  Needs no GPU."""
import numpy as np
import pytest

import rcnn_cases
import rpnloss_cases as RC


@pytest.fixture(scope="module")
def host():
    return RC.host_lib()


def test_key_is_the_samplers_key():
    for seed, b, r in ((0, 0, 0), (20240607, 3, 69119), (0xFFFFFFFF, 65534, (1 << 24) - 1), (17, 1, 255)):
        assert RC.sample_key(seed, b, r) == rcnn_cases.sample_key(seed, b, r)
        assert int(RC.sample_keys(seed, b, r + 1)[r]) == RC.sample_key(seed, b, r)


def test_case_list_covers_the_sizes():
    R = {c.id: RC.total(c) for c in RC.CASES}
    assert R["r1"] == 1 and R["g35-designed"] == 35 and R["a3-105"] == 105 and R["a15-300"] == 300
    assert (R["r255"], R["r256"], R["r257"]) == (255, 256, 257)
    assert len(RC.BY_ID["two-levels"].levels) == 2 and len(RC.BY_ID["five-levels"].levels) == 5
    assert R["quota-256-128"] == 6000 and 65536 < R["r69120"] < 2 * 65536
    assert {c.beta for c in RC.CASES} == {0.0, 0.1}


def test_designed_rows_do_what_they_were_designed_for():
    ref = RC.reference("g35-designed")
    lab, (pre, matched) = ref["lab"], (ref["lab"]["pre"], ref["lab"]["matched"])
    assert RC.margins_ok(ref)
    a = lambda x, y: y * 7 + x                                                    # anchor (x, y) of the 5 x 7 grid
    assert lab["promoted"] == [2, 4, 4, 0, 2]
    assert set(np.nonzero(pre[0] == 1)[0]) == {a(2, 2), a(3, 2)}                  # 0.6 twice: out of the ignore band
    assert set(np.nonzero(pre[1] == 1)[0]) == {a(2, 2), a(3, 2), a(2, 3), a(3, 3)}
    assert set(np.nonzero(pre[2] == 1)[0]) == {a(2, 2), a(3, 2), a(2, 3), a(3, 3)}
    assert (pre[3] == 0).all() and lab["counts"][3].tolist() == [0, 35, 0, 35]
    assert (matched[4] == 0).all() and (matched[1] == 0).all()                    # identical rows: the lowest; the absent row never
    q = RC.reference("quota-8-4")["lab"]["counts"][0]
    assert q[0] == 13 and q[2] == 4 and q[3] == 4
    q = RC.reference("quota-256-128")["lab"]["counts"][0]
    assert q[0] > 128 and q[2] == 128 and q[3] == 128
    q = RC.reference("none-present")["lab"]
    assert (q["pre"] == 0).all() and (q["matched"] == -1).all() and (q["counts"][:, 0] == 0).all()
    q = RC.reference("a3-105")["lab"]["counts"]
    assert (q[:, 0] < 128).all() and (q[:, 1] < 256 - q[:, 2]).all()              # both kinds below their quotas


@pytest.mark.parametrize("c", RC.CASES, ids=lambda c: c.id)
def test_host_labels_equal_the_oracle(host, c):
    ref = RC.reference(c.id)
    assert RC.margins_ok(ref)
    got, lab = RC.host_labels(host, c, ref), ref["lab"]
    for k in ("pre", "labels", "matched", "counts"):
        assert np.array_equal(got[k], lab[k]), (c.id, k, np.nonzero(got[k] != lab[k]))
    for b in range(c.B):                                                          # the sample against sorted() on (key, r)
        keys = RC.sample_keys(c.seed, b, RC.total(c))
        for kind, n in ((1, lab["counts"][b, 2]), (0, lab["counts"][b, 3])):
            want = sorted((int(keys[r]), int(r)) for r in np.nonzero(got["pre"][b] == kind)[0])[:n]
            assert sorted(r for _, r in want) == np.nonzero(got["labels"][b] == kind)[0].tolist()
        assert ((got["labels"][b] == -1) | (got["labels"][b] == got["pre"][b])).all()


def test_rows_dealt_to_two_levels_are_the_same_anchors(host):
    one, ref = RC.BY_ID["as-one"], RC.reference("as-one")
    two, ref2 = RC.split_rows(one, ref, 7)
    assert RC.total(two) == RC.total(one) and np.array_equal(RC.anchors(one, np.float32), RC.anchors(two, np.float32))
    a, b = RC.host_labels(host, one, ref), RC.host_labels(host, two, ref2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    la, lb = RC.host_loss(host, one, ref), RC.host_loss(host, two, ref2)
    assert float(abs(la["loss"][0] - lb["loss"][0])) <= 1e-6 * float(abs(la["loss"][0]))
    for k in ("grad_logits", "grad_deltas"):                                      # the same values, laid out level by level
        assert np.array_equal(np.sort(la[k].numpy()), np.sort(lb[k].numpy()))


@pytest.mark.parametrize("double", (False, True), ids=("float", "double"))
@pytest.mark.parametrize("c", RC.CASES, ids=lambda c: c.id)
def test_host_loss_and_gradients_match_the_oracle(host, c, double):
    ref = RC.reference(c.id)
    assert RC.margins_ok(ref)
    got = RC.host_loss(host, c, ref, double=double)
    assert not (got["grad_logits"] == RC.FSENT).any() and not (got["grad_deltas"] == RC.FSENT).any()      # every element written
    fails = RC.check_losses(c, ref, got, "host64" if double else "host32")
    assert not fails, fails
    if c.id == "none-present":
        assert got["loss"][2] == 0 and (got["grad_deltas"] == 0).all()

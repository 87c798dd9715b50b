"""The set-prediction detector stage without a GPU: the host build of csrc/gsr_setdet.h (the scalar source the kernels
compile) against the float64 PyTorch oracle of tests/setdet_cases.py, the oracle's own matcher against all permutations
and scipy, hand-derived literals, the hand-written backward against central finite differences of its own forward in
double, non-finite inputs in a child process, the output stage against a torch restatement of detr_detector.py:186-202,
and the same source as a stand-alone program under the address and undefined-behaviour sanitizers.  The hand-made inputs
of setdet_cases.py (exact ties, the backward's kinks, exact scores, one poisoned image of three) are held to the stated
rules here first; the device tests then demand the same of the kernels.

Bound on float errors (detloss_cases.bound): err = max|q - q64| / max|q64| of the host build may be at most 4 x the err of
the float32 oracle (the yardstick) for the same case and tensor, floor 2^-22, never above 1e-3.  Measured ratios are
recorded in DESIGN.md; every figure is printed before it is asserted."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import setdet_cases as SC


@pytest.fixture(scope="module")
def lib():
    return SC.host_lib()


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_the_cases_cover_what_they_claim(c):
    ref = SC.reference(c)
    o = ref["o64"]
    dets, counts, gap_score, gap_lead = ref["post"]
    print(f"{c.id}: gap_match {o['gap_match']:.3e} greedy_excess {o['greedy_excess']:.3e} gap_score {gap_score:.3e} "
          f"gap_lead {gap_lead:.3e} float32 cost err {ref['yard_cost_err']:.3e} kept {counts[:, 1].tolist()}")
    # the margin conditions: no decision sits where float32 rounding could cross it
    assert o["gap_match"] > SC.GAP_MATCH
    assert gap_score > SC.GAP_SCORE and gap_lead > SC.GAP_LEAD
    assert ref["yard_cost_err"] * 32 < SC.GAP_MATCH / 10
    assert ref["yard_match_equal"], "the float32 oracle matches differently: the seed is wrong"
    match, tgt, cls = o["match"].numpy(), o["tgt"].numpy(), ref["gt_cls"]
    assert match.shape == (c.B, c.M) and tgt.shape == (c.B, c.Q) and ref["logits"].shape == (c.B, c.Q, c.C + 1)
    present = (cls >= 0) & (cls < c.C)
    assert ((match >= 0) == present).all()
    for b in range(c.B):                                                   # one-to-one, and tgt is its inverse
        qs = match[b][present[b]]
        assert len(set(qs.tolist())) == len(qs) and (tgt[b, qs] == np.nonzero(present[b])[0]).all()
        assert (tgt[b] >= 0).sum() == present[b].sum()
    if c.id == "one":
        assert (c.B, c.Q, c.C, c.M) == (1, 1, 1, 1) and match[0, 0] == 0
    if c.id == "ragged":
        assert c.Q % 64 != 0
        assert not present[1].any() and (tgt[1] == -1).all()               # one image with every row absent
        assert cls[2, 3] >= c.C and match[2, 3] == -1                      # a class past the head's is absent too
        assert not present[0, 1] and present[0, 0] and present[0, 2]       # present rows are not contiguous
    if c.id == "contested":
        gt = ref["gt_boxes"]
        assert (np.abs(gt - gt[:, :1]).max() / np.abs(gt).max()) < 0.1     # near-duplicates of one box
        assert o["greedy_excess"] > SC.GAP_MATCH                           # rows taken greedily in order cost more
    if c.id == "full-rows":
        assert c.Q == c.M == 32 and (tgt >= 0).all()                       # every query matched: no no-object term
    if c.id == "no-gt":
        assert not present.any() and (tgt == -1).all()
        assert o["loss"][1] == 0 and o["loss"][2] == 0 and (o["grad_boxes"] == 0).all()
    if c.id == "saturated":
        assert np.abs(ref["logits"]).min() == 80.0 and np.abs(ref["logits"]).max() == 80.0
        x1 = ref["boxes"][..., 0] - 0.5 * ref["boxes"][..., 2]
        x2 = ref["boxes"][..., 0] + 0.5 * ref["boxes"][..., 2]
        assert (x1 == 0).any() and (x2 == 1).any()
        assert all(torch.isfinite(o[k]).all() for k in SC.COMPARED)
    if c.id == "wide":
        assert c.Q > 256 * 3 and c.Q % 256 != 0                            # several passes of the match's workgroup, a ragged last
    claim = SC.EDGE_CLAIMS.get(c.id)
    if claim is not None:                                                  # the edge cases: what the kernels add to the source
        assert c.kind == "plain" and SC.covers(c, ref)
        assert (c.B * c.Q) % 4 == claim["bq_mod4"]                         # the cost kernel's last workgroup: 4 queries each
        assert present.all() and (match >= 0).all()                        # every row present and matched
        if "images_above" in claim:
            assert c.B > claim["images_above"] == 256                      # block_matched strides 256 threads over B
        if "term_blocks_above" in claim:
            assert SC.term_blocks(c) > claim["term_blocks_above"] == 256   # slab_sum strides 256 threads over the blocks
        if c.id == "limits":
            assert (c.Q, c.C, c.M) == (1024, 1024, 32) and SC.term_blocks(c) == 1025
        assert (counts[:, 1] > 0).any() and (counts[:, 1] < c.Q).any()     # a query kept and a query dropped in the batch
    elif c.kind in ("plain", "ragged") and c.Q > 1:
        assert (counts[:, 1] > 0).all() and (counts[:, 1] < c.Q).all()     # the output stage keeps some queries, not all


def test_every_edge_case_is_a_case():
    assert set(SC.EDGE_CLAIMS) <= set(SC.BY_ID) and len(SC.BY_ID) == len(SC.CASES)
    assert [c.id for c in SC.CASES[:8]] == ["one", "tiny", "ragged", "contested", "full-rows", "no-gt", "saturated", "wide"]


# ---- the oracle's matcher on its own ----------------------------------------------------------------------------------------
def test_oracle_matcher_against_all_permutations():
    rng = np.random.default_rng(11)
    for trial in range(60):
        M = int(rng.integers(1, 5))
        Q = int(rng.integers(M, 9))
        cost = rng.normal(0, 2, (M, Q))
        rows = [m for m in range(M) if rng.uniform() < 0.8] or [0]
        r2c, total = SC.solve_assignment(cost, rows)
        perm, best = SC.brute_force(cost, rows)
        assert abs(total - best) <= 1e-12 * max(1.0, abs(best)), (trial, total, best)
        assert [int(r2c[m]) for m in rows] == list(perm)                   # random costs: the optimum is unique
        assert all(r2c[m] == -1 for m in range(M) if m not in rows)


def test_oracle_matcher_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(12)
    for M, Q in ((1, 1), (3, 7), (6, 16), (32, 32), (8, 900), (32, 100)):
        cost = rng.normal(0, 2, (M, Q))
        r2c, total = SC.solve_assignment(cost, list(range(M)))
        ri, ci = opt.linear_sum_assignment(cost)
        assert np.array_equal(ci, r2c[ri]) and abs(total - cost[ri, ci].sum()) <= 1e-12 * max(1.0, abs(total))
    for c in SC.CASES:                                                     # and on the cases' own cost matrices
        ref = SC.reference(c)
        cost, cls = ref["o64"]["cost"].numpy(), ref["gt_cls"]
        for b in range(c.B):
            rows = [m for m in range(c.M) if 0 <= cls[b, m] < c.C]
            if rows:
                ri, ci = opt.linear_sum_assignment(cost[b][rows])
                assert np.array_equal(ci, ref["o64"]["match"].numpy()[b][rows]), (c.id, b)


# ---- the host build -----------------------------------------------------------------------------------------------------------
def check_against_oracle(c, got, ref, who):
    """match and tgt integer-equal, loss / grad_logits / grad_boxes within the bound; prints each figure first."""
    o = ref["o64"]
    assert np.array_equal(np.asarray(got["match"]), o["match"].numpy()), f"{who} {c.id}: match differs"
    assert np.array_equal(np.asarray(got["tgt"]), o["tgt"].numpy()), f"{who} {c.id}: tgt differs"
    fails = []
    for k in SC.COMPARED:
        if got.get(k) is None:
            continue
        e, y = SC.err(got[k], o[k]), ref["yard"][k]
        b = SC.bound(y)
        print(f"{who} {c.id} {k}: err {e:.3e} yardstick {y:.3e} ratio {e / max(y, 1e-30):.2f} bound {b:.3e}")
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, f"{who} {c.id}: {fails}"


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_host_build_against_the_oracle(lib, c):
    ref = SC.reference(c)
    got = SC.host_run(lib, ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"])
    assert np.isfinite(got["grad_logits"]).all() and np.isfinite(got["grad_boxes"]).all() and np.isfinite(got["loss"]).all()
    check_against_oracle(c, got, ref, "host")
    e = np.abs(got["cost"].astype(np.float64) - ref["o64"]["cost"].numpy()).max()
    print(f"host {c.id} cost: max abs err {e:.3e}")
    assert e * 32 < SC.GAP_MATCH / 10
    # without the gradients the loss is the same bits
    again = SC.host_run(lib, ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"], want_grad=False)
    assert again["loss"].tobytes() == got["loss"].tobytes() and np.array_equal(again["match"], got["match"])
    # unmatched queries: zero box gradients
    assert (got["grad_boxes"][got["tgt"] < 0] == 0).all()


def test_double_host_build_equals_the_oracle(lib):
    """The same code in double against the float64 oracle: what is left is rounding alone."""
    for cid in ("ragged", "contested"):
        ref = SC.reference(SC.BY_ID[cid])
        got = SC.host_run(lib, ref["logits"], ref["boxes"], ref["gt_boxes"], ref["gt_cls"], double=True)
        assert np.array_equal(got["match"], ref["o64"]["match"].numpy()) and np.array_equal(got["tgt"], ref["o64"]["tgt"].numpy())
        for k in SC.COMPARED:
            assert SC.err(got[k], ref["o64"][k]) < 1e-12, (cid, k)
        assert np.abs(got["cost"] - ref["o64"]["cost"].numpy()).max() < 1e-12


# ---- hand-derived literals ------------------------------------------------------------------------------------------------------
# B = Q = C = M = 1 in a 640 x 480 frame.  The query's box (0.5, 0.5, 0.5, 0.5) is (0.25, 0.25, 0.75, 0.75); the gt box
# (320, 120, 480, 360) px is (0.625, 0.5, 0.25, 0.5) normalised, (0.5, 0.25, 0.75, 0.75) as corners -- the right half of the
# query's box.  |box - gt| = (0.125, 0, 0.25, 0): l1 = 0.375.  inter = 0.125, union = 0.25, iou = 0.5; the enclosing box is
# the query's, encl = union: giou = 0.5, the term 1 - 0.5.  logits (0, 0): ce = ln 2, W = 1, n = 1.
ONE = dict(logits=np.zeros((1, 1, 2)), boxes=np.array([[[0.5, 0.5, 0.5, 0.5]]]), gt_boxes=np.array([[[320.0, 120.0, 480.0, 360.0]]]),
           gt_cls=np.array([[0]], np.int32))


def test_literals_for_one_query_and_one_row(lib):
    for double in (False, True):
        got = SC.host_run(lib, double=double, **ONE)
        assert got["match"].tolist() == [[0]] and got["tgt"].tolist() == [[0]]
        tol = 1e-15 if double else 2.0 ** -22
        assert abs(got["loss"][0] - math.log(2.0)) <= tol
        assert got["loss"][1] == 0.375 and got["loss"][2] == 0.5           # every value is a short binary fraction
        assert abs(got["loss"][3] - (math.log(2.0) + 5 * 0.375 + 2 * 0.5)) <= 4 * tol
        assert got["cost"][0, 0, 0] == -0.5 + 5 * 0.375 - 2 * 0.5
        assert got["grad_logits"].tolist() == [[[-0.5, 0.5]]]              # p - onehot
    # L1 alone: sign(0) = 0 on the two coordinates that agree
    got = SC.host_run(lib, w=(1.0, 5.0, 0.0), **ONE)
    assert got["grad_boxes"].tolist() == [[[-5.0, 0.0, 5.0, 0.0]]]
    # GIoU alone: x2, y1 and y2 of the two boxes are equal, so every max / min there shares its gradient in halves -- against
    # torch's autograd, which does the same
    got = SC.host_run(lib, double=True, w=(1.0, 0.0, 2.0), **ONE)
    o = SC.oracle(ONE["logits"], ONE["boxes"], ONE["gt_boxes"], ONE["gt_cls"], w=(1.0, 0.0, 2.0))
    assert np.abs(got["grad_boxes"] - o["grad_boxes"].numpy()).max() < 1e-14 and np.abs(got["grad_boxes"]).max() > 0.1
    # an unmatched query: the no-object class with weight eos_coef; W = eos_coef, so ce = ln 2 again and no box terms
    got = SC.host_run(lib, ONE["logits"], ONE["boxes"], ONE["gt_boxes"], np.array([[-1]], np.int32), double=True)
    assert got["match"].tolist() == [[-1]] and got["tgt"].tolist() == [[-1]]
    assert abs(got["loss"][0] - math.log(2.0)) <= 1e-15 and got["loss"][1] == 0 and got["loss"][2] == 0
    assert got["grad_logits"].tolist() == [[[0.5, -0.5]]] and (got["grad_boxes"] == 0).all()


def test_equal_costs_go_to_the_lowest_query(lib):
    """Two rows of one class with the same box, four identical queries: every assignment costs the same.  The stated rule
    gives row 0 query 0 and row 1 query 1 (the lowest column among equal candidates, rows inserted in order)."""
    logits = np.zeros((1, 4, 3))
    boxes = np.tile(np.array([0.5, 0.5, 0.25, 0.25]), (1, 4, 1))
    gt = np.tile(np.array([160.0, 120.0, 480.0, 360.0]), (1, 2, 1))
    got = SC.host_run(lib, logits, boxes, gt, np.array([[1, 1]], np.int32))
    assert got["match"].tolist() == [[0, 1]] and got["tgt"].tolist() == [[0, 1, -1, -1]]


@pytest.mark.parametrize("kind", SC.TIE_KINDS)
def test_exact_ties_follow_the_stated_rule(lib, kind):
    """setdet_cases.tie_inputs on the serial match: what the device test then demands of the lane-dealt one.  Identical
    queries and rows: row m takes query m.  A cheaper block of equal candidates at queries 253..264: its first six.
    Duplicated prototypes: the distinct costs of a row lie further apart than GAP_MATCH in the float64 oracle (so float32
    keeps every order and every equality), the match is an optimum of the oracle's cost matrix and one-to-one."""
    ref = SC.tie_reference(kind)
    got = SC.host_run(lib, *ref["inputs"])
    print(f"ties {kind}: distinct costs of a row at least {ref['gap']:.3e} apart; the oracle's own match {ref['match'].tolist()}")
    assert ref["gap"] > SC.GAP_MATCH
    if kind == "identical":
        assert got["match"].tolist() == [[0, 1, 2, 3, 4, 5]]
    if kind == "block":
        assert got["match"].tolist() == [list(SC.TIE_BLOCK)[:SC.TIE_M]] == [[253, 254, 255, 256, 257, 258]]
    if kind == "prototypes":
        x, bx, gt, cls = ref["inputs"]
        protos = {(x[0, q].tobytes(), bx[0, q].tobytes()) for q in range(SC.TIE_Q)}
        assert len(protos) == 5 and len({(gt[0, m].tobytes(), int(cls[0, m])) for m in range(SC.TIE_M)}) == 4
        for r in ref["cost"]:                                              # a row's cost has one value per prototype
            assert len(np.unique(r)) == 5
        # the rule on this input: every row takes the lowest free query of its cheapest prototype
        want, taken = [], set()
        for r in ref["cost"]:
            q = min(q for q in range(SC.TIE_Q) if r[q] == r.min() and q not in taken)
            want.append(q)
            taken.add(q)
        assert got["match"].tolist() == [want]
    SC.check_tie("host", kind, got, got["match"])
    d = SC.host_run(lib, *ref["inputs"], double=True, want_grad=False)
    assert np.array_equal(d["match"], got["match"]) and np.array_equal(d["tgt"], got["tgt"])


def test_backward_at_its_kinks(lib):
    """setdet_cases.kink_inputs: the matched box equal to its gt, touching it, disjoint, containing it, inside with a shared
    edge, of zero size.  torch's autograd follows the contract's conventions there (ties of max / min in halves, clamps
    passing at 0, sign(0) = 0), so the usual bound against the float64 oracle holds; and where every step is exact the
    values are literals: one image alone has n = 1, so k_l1 = 5 and k_giou = 2 exactly."""
    inputs = SC.kink_inputs()
    o = SC.oracle(*inputs, want_gap=True)
    got = SC.host_run(lib, *inputs)
    print(f"kinks: gap_match {o['gap_match']:.3e}")
    assert o["gap_match"] > SC.GAP_MATCH and (o["match"] == 0).all()
    assert np.array_equal(got["match"], o["match"].numpy()) and np.array_equal(got["tgt"], o["tgt"].numpy())
    assert np.isfinite(got["grad_boxes"]).all() and np.isfinite(got["loss"]).all()
    SC.check_with_match_frozen("host kinks", got, inputs)
    names = [k[0] for k in SC.KINKS]
    assert (got["grad_boxes"][names.index("equal"), 0] == 0).all() and (got["grad_boxes"][:, 1] == 0).all()
    literals = {"equal": [0.0, 0.0, 0.0, 0.0], "inside-shared-edge": [-7.25, 0.0, -5.875, -7.0], "zero-size": [0.0, 0.0, -5.0, -5.0]}
    assert set(literals) == set(SC.KINK_EXACT)
    for name, want in literals.items():
        one = SC.kink_inputs(name)
        for double in (False, True):
            g = SC.host_run(lib, *one, double=double)
            assert g["match"].tolist() == [[0]] and g["grad_boxes"][0, 0].tolist() == want, (name, double)
        assert SC.oracle(*one)["grad_boxes"][0, 0].tolist() == want, name


def test_postprocess_at_exact_scores_and_limits(lib):
    """The output stage at exact scores (a class tie at 0.5, a score exactly at conf_thr, NaN and -inf logits), at max_det = 1 and
    1024 and with all and none of 65 queries kept: setdet_cases.exact_score_expectations, shared with the device test."""
    SC.exact_score_expectations(lambda x, bx, thr, max_det: SC.host_post(lib, x, bx, thr=thr, max_det=max_det))


# ---- the hand-written backward against its own forward ------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["tiny", "contested"])
def test_gradient_equals_the_finite_difference_of_the_forward(lib, cid):
    """In double, with the match frozen (what the contract's backward holds constant): every box coordinate of a matched
    query and 60 sampled logits.  Central differences with h = 1e-6 on a double forward: truncation ~ h^2 |f'''| ~ 1e-11,
    rounding ~ 1e-16 |total| / h ~ 1e-9; the tolerance is 1e-6 of the largest gradient of the tensor."""
    ref = SC.reference(SC.BY_ID[cid])
    x, bx = ref["logits"].astype(np.float64), ref["boxes"].astype(np.float64)
    base = SC.host_run(lib, x, bx, ref["gt_boxes"], ref["gt_cls"], double=True)
    frozen = (base["match"], base["tgt"])
    again = SC.host_run(lib, x, bx, ref["gt_boxes"], ref["gt_cls"], double=True, frozen=frozen)
    assert again["loss"].tobytes() == base["loss"].tobytes() and again["grad_boxes"].tobytes() == base["grad_boxes"].tobytes()
    rng = np.random.default_rng(5)
    h = 1e-6

    def total(xv, bv):
        return SC.host_run(lib, xv, bv, ref["gt_boxes"], ref["gt_cls"], double=True, want_grad=False, frozen=frozen)["loss"][3]

    worst_b, worst_l = 0.0, 0.0
    for b, q in np.argwhere(base["tgt"] >= 0):
        for k in range(4):
            bp, bm = bx.copy(), bx.copy()
            bp[b, q, k] += h
            bm[b, q, k] -= h
            worst_b = max(worst_b, abs((total(x, bp) - total(x, bm)) / (2 * h) - base["grad_boxes"][b, q, k]))
    for _ in range(60):
        i = tuple(rng.integers(0, n) for n in x.shape)
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        worst_l = max(worst_l, abs((total(xp, bx) - total(xm, bx)) / (2 * h) - base["grad_logits"][i]))
    sb, sl = np.abs(base["grad_boxes"]).max(), np.abs(base["grad_logits"]).max()
    print(f"finite differences {cid}: boxes worst {worst_b:.3e} of {sb:.3e}, logits worst {worst_l:.3e} of {sl:.3e}")
    assert worst_b <= 1e-6 * sb and worst_l <= 1e-6 * sl


# ---- non-finite inputs: the loops end and the indices stay in range -------------------------------------------------------------
_POISON = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import setdet_cases as SC
lib = SC.host_lib()
for cid in ("ragged", "contested", "full-rows", "wide"):
    c = SC.BY_ID[cid]
    logits, boxes, gtb, gtc = SC.make_inputs(c)
    rng = np.random.default_rng(4)
    for frac in (0.05, 0.5, 1.0):
        x, bx = logits.copy(), boxes.copy()
        for a in (x, bx):
            bad = rng.uniform(0, 1, a.shape)
            a[bad < frac * 0.4] = np.nan
            a[(bad >= frac * 0.4) & (bad < frac * 0.7)] = np.inf
            a[(bad >= frac * 0.7) & (bad < frac)] = -np.inf
        got = SC.host_run(lib, x, bx, gtb, gtc)
        present = (gtc >= 0) & (gtc < c.C)
        assert got["match"].min() >= -1 and got["match"].max() < c.Q, (cid, frac)
        assert got["tgt"].min() >= -1 and got["tgt"].max() < c.M, (cid, frac)
        assert ((got["match"] >= 0) == present).all(), (cid, frac)
        for b in range(c.B):
            qs = got["match"][b][present[b]]
            assert len(set(qs.tolist())) == len(qs), (cid, frac)
        dets, counts = SC.host_post(lib, x, bx)
        assert counts.min() >= 0 and counts.max() <= c.Q
# one poisoned image of three: the other two keep the clean run's bits (the inputs of the device test)
for c in SC.NONFINITE_CASES:
    logits, boxes, gtb, gtc = SC.make_inputs(c)
    assert c.B == 3 and ((gtc >= 0) & (gtc < c.C)).all()
    clean = SC.host_run(lib, logits, boxes, gtb, gtc)
    for frac in SC.NONFINITE_FRACS:
        x, bx = SC.poisoned_inputs(c, frac)
        assert np.array_equal(x[[0, 2]], logits[[0, 2]]) and np.array_equal(bx[[0, 2]], boxes[[0, 2]])
        share = 1 - np.isfinite(x[1]).mean()
        assert abs(share - frac) < 0.1 and np.isnan(x[1]).any() and np.isposinf(x[1]).any() and np.isneginf(x[1]).any()
        got = SC.host_run(lib, x, bx, gtb, gtc)
        SC.check_poisoned(f"host {c.id} {frac}", c, got, clean, gtc, SC.host_post(lib, x, bx)[1])
print("poison ok")
"""


def test_non_finite_inputs_return_with_every_index_in_range(lib):
    """NaN and +-inf in logits and boxes give unspecified floats, but the match stays one-to-one and in range and every
    loop ends: run in a child process so that a loop that did not end would be cut off instead of hanging the suite.  With
    one image of three poisoned, the other two keep the bits of the clean run (setdet_cases.check_poisoned)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _POISON, here], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout + r.stderr


# ---- the output stage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.id)
def test_postprocess_equals_the_reference_restated(lib, c):
    """Kept queries, their order, classes and counts are integer-equal; the boxes are the same float32 operations in the same
    order, so they are equal bit for bit; the score is a float32 softmax taken in another summation order: within
    setdet_cases.score_tol."""
    ref = SC.reference(c)
    want, wcounts, _, _ = ref["post"]
    dets, counts = SC.host_post(lib, ref["logits"], ref["boxes"])
    assert np.array_equal(counts, wcounts)
    assert np.array_equal(dets[..., :4], want[..., :4]) and np.array_equal(dets[..., 5], want[..., 5])
    print(f"host postprocess {c.id}: score max abs diff {np.abs(dets[..., 4] - want[..., 4]).max():.3e} tol {SC.score_tol(c.C):.3e}")
    assert np.abs(dets[..., 4] - want[..., 4]).max() <= SC.score_tol(c.C)
    for b in range(c.B):
        assert (dets[b, counts[b, 0]:] == 0).all()
    # fewer rows than kept queries: the first max_det in query order, counts = (max_det, above)
    if wcounts[:, 1].max() > 1:
        k = int(wcounts[:, 1].max()) - 1
        d2, c2 = SC.host_post(lib, ref["logits"], ref["boxes"], max_det=k)
        assert np.array_equal(c2[:, 1], wcounts[:, 1]) and np.array_equal(c2[:, 0], np.minimum(wcounts[:, 1], k))
        assert np.array_equal(d2, dets[:, :k])


# ---- the same source as a program under the sanitizers ----------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    src, _ = SC.host_sources()
    exe = str(tmp_path / "setdet_host_san")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DSETDET_MAIN", "-I", SC.CSRC, src, "-o", exe], check=True)
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        for c in SC.CASES:
            ref = SC.reference(c)
            f.write(np.array([c.B, c.Q, c.C, c.M], np.int32).tobytes())
            f.write(np.array(SC.FRAME, np.float32).tobytes())
            for k in ("logits", "boxes", "gt_boxes", "gt_cls"):
                f.write(np.ascontiguousarray(ref[k]).tobytes())
    r = subprocess.run([exe, str(data)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"cases {len(SC.CASES)}"
    for k, c in enumerate(SC.CASES):
        want = SC.reference(c)["o64"]["match"].numpy().reshape(-1).tolist()
        for tag in ("match", "match64"):
            line = next(ln for ln in lines if ln.startswith(f"case {k} {tag} "))
            assert [int(v) for v in line.split()[3:]] == want, (c.id, tag)

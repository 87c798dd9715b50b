"""The RPN proposal stage without a GPU: the oracle of tests/rpn_cases.py holds its margins and the properties its cases
are there for, its order is plain Python's sorted() on (-logit, index), gsplat_attack's cell_anchors equals hand-written
literals, and the host build of csrc/gsr_rpn.h equals the oracle -- kept slots, counts, levels and ranks integer-equal, scores
bit-equal, decoded boxes within the float32 yardstick's bound."""
import math

import numpy as np
import pytest

import rpn_cases as PC


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_oracle_margins(c):
    ref = PC.reference(c)
    print(f"{c.id}: iou gap {ref['iou_gap']:.3e} size gap {ref['size_gap']:.3e} logit gap {ref['logit_gap']:.3e} "
          f"kept {ref['nms']['counts'].tolist()} walked {ref['nms']['walked'].tolist()} of {ref['nms']['n_order'].tolist()}")
    assert PC.margins_ok(c, ref)
    if c.exact:
        for lv in PC.inputs(c):
            assert not lv.deltas.any() and np.array_equal(lv.cell, np.rint(lv.cell))
            assert all(float(v).is_integer() for v in c.frame) and c.thr in (0.5, 0.75)
    else:
        assert c.thr == 0.7 and ref["N"] <= 300
        assert np.array_equal(PC.inputs(c)[0].cell, PC.real_cell_anchors())


def test_cell_anchors_literals():
    from gsplat_attack.proposals import cell_anchors
    got = cell_anchors((32,), (0.5, 1.0, 2.0))
    lit = np.array([[-22.627416997969522, -11.313708498984761, 22.627416997969522, 11.313708498984761],
                    [-16.0, -16.0, 16.0, 16.0],
                    [-11.313708498984761, -22.627416997969522, 11.313708498984761, 22.627416997969522]]).astype(np.float32)
    assert got.dtype.is_floating_point and got.numpy().dtype == np.float32 and got.numpy().tobytes() == lit.tobytes()
    assert cell_anchors(PC.SIZES, PC.RATIOS).numpy().tobytes() == PC.real_cell_anchors().tobytes()
    with pytest.raises(ValueError):
        cell_anchors((), (1.0,))


@pytest.mark.parametrize("c", [c for c in PC.CASES if c.id in ("tie-at-k", "short-level", "float-min0", "two-levels")], ids=lambda c: c.id)
def test_oracle_order_is_pythons_sorted(c):
    ref = PC.reference(c)
    for l, lv in enumerate(PC.inputs(c)):
        n = PC.slots_of(c)[l]
        for b in range(c.B):
            v = PC.flat_logits(lv.logits[b])
            want = sorted((i for i in range(v.size) if not math.isnan(v[i])), key=lambda i: (-float(v[i]), i))[:n]
            got = ref["index"][l][b]
            assert got[:len(want)].tolist() == want and (got[len(want):] == -1).all()
    # ... and the walk's: (-score, slot) over the slots that take part
    cs, cl = ref["cand_scores"], ref["cand_level"]
    for b in range(c.B):
        want = sorted((s for s in range(cs.shape[1]) if cl[b, s] >= 0), key=lambda s: (-float(cs[b, s]), s))
        assert PC.walk_order(cs[b], cl[b]).tolist() == want


def test_case_properties():
    by = {c.id: c for c in PC.CASES}
    # the k-th place falls inside a group of equal logits; +0.0 and -0.0 are both among the logits
    for cid in ("tie-at-k", "c4-thr50-post4096"):
        c = by[cid]
        lv, ref = PC.inputs(c)[0], PC.reference(c)
        split = []
        for b in range(c.B):
            v = PC.flat_logits(lv.logits[b])
            idx = ref["index"][0][b]
            last = v[idx[-1]]
            split.append(int((v == last).sum()) > int((v[idx] == last).sum()))
        assert any(split), cid
        if cid == "c4-thr50-post4096":
            assert split[0]                                    # the quantised image
    z = PC.inputs(by["tie-at-k"])[0].logits
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    assert PC.slots_of(by["short-level"]) == [105] and 105 % 64 != 0
    assert 3 * 150 * 150 > 1 << 16 and len(np.unique(PC.inputs(by["all-equal"])[0].logits)) == 1
    assert PC.reference(by["full-slots"])["N"] == PC.MAX_SLOTS
    # the C4 shape: one image walks into the last chunk without hitting post_topk, one stops early
    for cid in ("c4-thr50-post4096", "c4-thr75-post2000"):
        c = by[cid]
        assert (c.B, c.levels, c.pre_topk) == (2, PC.C4, 12000)
        lg = PC.inputs(c)[0].logits
        assert 100 < len(np.unique(lg[0])) < 1000 and len(np.unique(lg[1])) == lg[1].size
    n = PC.reference(by["c4-thr50-post4096"])["nms"]
    last_chunk = (n["n_order"] - 1) // 64 * 64
    to_end = (n["walked"] > last_chunk) & (n["counts"] < 4096)
    early = (n["counts"] == 4096) & (n["walked"] <= last_chunk)
    assert to_end.any() and early.any(), (n["walked"], n["counts"])
    m = PC.reference(by["c4-thr75-post2000"])["nms"]
    assert ((m["counts"] == 2000) & (m["walked"] < m["n_order"] - 64)).any()
    # two levels: coincident boxes on different levels both survive
    t = PC.reference(by["two-levels"])
    found = False
    for b in range(2):
        keep = t["nms"]["keep"][b][: t["nms"]["counts"][b]]
        bx, lv = t["cand_boxes"][b][keep], t["cand_level"][b][keep]
        for i in np.nonzero(lv == 1)[0]:
            found = found or bool(((bx[lv == 0] == bx[i]).all(1)).any())
    assert found


def test_nms_case_properties():
    by = {c.id: c for c in PC.NMS_CASES}
    assert sorted({PC.nms_inputs(c)[1].shape[1] for c in PC.NMS_CASES if c.gen != "chains"}) == [1, 63, 64, 65, 129, 4097, 16384]
    # chains: c stays although b overlaps it, because a suppressed b -- in one chunk, over three chunks, over two
    bx, sc, lv, marks = PC._chain_slots()
    ref = PC.nms_reference(by["chains"])
    for b in range(2):
        kept = set(ref["keep"][b][: ref["counts"][b]].tolist())
        ch = marks["chains"]
        assert len(ch) == 9
        for a_, b_, c_ in (ch[0:3], ch[3:6], ch[6:9]):
            assert a_ in kept and b_ not in kept and c_ in kept
        order = PC.walk_order(sc, lv).tolist()
        chunks = [[order.index(s) // 64 for s in tri] for tri in (ch[0:3], ch[3:6], ch[6:9])]
        assert chunks[0][0] == chunks[0][2] and len(set(chunks[1])) == 3 and chunks[2][0] != chunks[2][1] == chunks[2][2]
        t0 = marks["twin0"]
        assert t0 in kept and t0 + 1 not in kept and {t0 + 2, t0 + 3} <= kept and len(sc) - 1 not in kept
    # the caps: inside a chunk, and at 4096
    r = PC.nms_reference(by["n129-cap-midchunk"])
    assert (r["counts"] == 37).all() and (r["walked"] % 64 != 0).all() and (r["walked"] < r["n_order"]).all()
    r = PC.nms_reference(by["n129-cap-second-chunk"])
    assert (r["counts"] == 70).all() and (r["walked"] == 70).all()
    r = PC.nms_reference(by["n4097-all-kept-cap4096"])
    assert (r["counts"] == 4096).all() and (r["walked"] == 4096).all() and (r["n_order"] == 4097).all()
    r = PC.nms_reference(by["n16384"])
    assert (r["counts"] == 4096).all()
    for cid in ("n63-thr75", "n64", "n65-thr75", "n129"):
        bxs, scs, lvs, _, _ = PC.nms_inputs(by[cid])
        r = PC.nms_reference(by[cid])
        assert (lvs == -1).any() and (lvs == 0).any() and (lvs == 1).any()                    # slots of level -1 interleaved
        assert (r["counts"] < (lvs >= 0).sum(1)).all()                                         # something was suppressed


@pytest.mark.parametrize("c", PC.NMS_CASES, ids=lambda c: c.id)
def test_host_nms_equals_the_oracle(c):
    bx, sc, lv, thr, post = PC.nms_inputs(c)
    ref, got = PC.nms_reference(c), PC.host_nms(PC.host_lib(), bx, sc, lv, thr, post)
    assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["keep"], ref["keep"])
    assert got["scores"].tobytes() == ref["scores"].tobytes() and got["proposals"].tobytes() == ref["proposals"].astype(np.float32).tobytes()


@pytest.mark.parametrize("c", PC.CASES, ids=lambda c: c.id)
def test_host_build_equals_the_oracle(c):
    ref, got = PC.reference(c), PC.host_propose(c)
    assert PC.margins_ok(c, ref)
    for l in range(len(c.levels)):
        assert np.array_equal(got["index"][l], ref["index"][l]), f"{c.id}: ranks of level {l}"
    assert np.array_equal(got["cand_level"], ref["cand_level"])
    assert got["cand_scores"].tobytes() == ref["cand_scores"].tobytes()
    PC.box_check(f"host {c.id} cand_boxes", got["cand_boxes"], ref["cand_boxes"], ref["cand_boxes32"])
    if c.exact:
        assert got["cand_boxes"].tobytes() == ref["cand_boxes"].astype(np.float32).tobytes()
    n = ref["nms"]
    assert np.array_equal(got["nms"]["counts"], n["counts"]) and np.array_equal(got["nms"]["keep"], n["keep"])
    assert got["nms"]["scores"].tobytes() == n["scores"].tobytes()
    PC.box_check(f"host {c.id} proposals", got["nms"]["proposals"], n["proposals"], PC.proposals32(ref))

"""Child process of tests/test_gpu_list_edges.py::test_other_segment_lengths_in_a_fresh_process: families A and B under the
GSR_SEG_SHIFT of its environment, default flags and bwd_split(4), held to the checks of the parent's single-view test;
writes the maxima as JSON to argv[1].  Exits non-zero on the first failed check."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import list_edge_scenes as S  # noqa: E402
import test_gpu_list_edges as G  # noqa: E402


def main(dst):
    D = G._D()
    dev = torch.device("cuda:0")
    worst, records, cases = {}, {}, 0
    for key in ("A", "B"):
        sc = S.get(key)
        r64, r32 = S.oracle_run(sc, 0), S.oracle_run(sc, 0, torch.float32)
        for name, flags in (("default", 0), ("bwd4", D.flag_bwd_split(4))):
            res, grads = G.run_single(D, sc, flags, "raw", False, False, "C", dev)
            tag = f"{sc.name} / shift {G.seg_shift()} / {name}"
            G.check_forward(tag, sc, 0, res, r64, r32, False, worst)
            ref64, ref32 = G.refs_for(sc, 0, "C", list(grads))
            G.check_grads(tag, grads, ref64, ref32, S.dead_gaussians(sc), G.first_entries(sc.facts[0]), worst)
            records[sc.name] = res["records"]
            cases += 1
    with open(dst, "w") as fh:
        json.dump(dict(seg_shift=G.seg_shift(), cases=cases, records=records, worst=worst), fh)


if __name__ == "__main__":
    main(sys.argv[1])

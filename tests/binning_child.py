"""Child process of tests/test_gpu_binning_variants.py: the binning front end under the GSR_DEPTH_PASSES / GSR_RS_ROUNDS of
its environment (both are read once per process).  Runs the cases of CASES with the helpers of test_gpu_binning.py, checks
after every case that each forward of the case reported the variants the environment asks for, and writes what it ran as
JSON to argv[1].  Exits non-zero on the first failed check."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "3d-gaussian-splat-attack_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import test_gpu_binning as G  # noqa: E402

CASES = ([f"depth/{d}" for d in G.DEPTH_DISTS + [G.WIDEST]] + [f"live/{v}" for v in G.LIVE_COUNTS]
         + ["tiles-per-rank", "oracle/hydrant-1k"])


def expected_variants():
    """(depth passes, chunk rounds) every forward of this process must report: the scenes here are far below the sizes at
    which the library picks the large variants by itself."""
    passes = int(os.environ.get("GSR_DEPTH_PASSES", "3"))
    rounds = int(os.environ.get("GSR_RS_ROUNDS", "8"))
    assert passes in (3, 4) and rounds in (8, 16)
    return passes, rounds


def main(dst):
    D = G._hip()
    dev = torch.device("cuda:0")
    passes, rounds = expected_variants()
    # every context this process creates, whichever helper made it
    holders = []
    init = D._CtxHolder.__init__

    def recording_init(self, lib, handle):
        init(self, lib, handle)
        holders.append(self)
    D._CtxHolder.__init__ = recording_init

    ran, forwards, widths = [], 0, {}
    for case in CASES:
        kind, _, arg = case.partition("/")
        if kind == "depth":
            out = G._depth_order_case(D, dev, arg)
            w = int(D.export_state(out["render"], "dv")[G.DV_W])
            widths[arg] = w
            if arg == G.WIDEST:                              # 30+ bits of key range: 10/11-bit digits in three passes, 8 in four
                assert (w <= 8) if passes == 4 else (w >= 10), f"digit width {w} under {passes} passes"
            assert w <= (8 if passes == 4 else 11)
        elif kind == "live":
            out = G._live_count_case(D, dev, int(arg))
        elif kind == "tiles-per-rank":
            out = G._tiles_per_rank_case(D, dev)
        else:
            nfrag, N = G._tile_list_parity(arg)
            assert nfrag == 0 and N > 1000, (nfrag, N)       # no fragile Gaussian, nothing excused
            out = None
        assert holders, f"{case}: no forward ran"
        for h in holders:
            n, got = h.info(0), (h.info(G.INFO_DEPTH_PASSES), h.info(G.INFO_TILE_ROUNDS))
            assert got == (passes, rounds if n > 0 else 0), f"{case}: a forward of {n} pairs took {got}, asked for {(passes, rounds)}"
            assert h.info(G.INFO_SCAN_ITEMS) == 8 and h.info(G.INFO_GROUP_SUMS) == 0
        forwards += len(holders)
        del out
        holders.clear()
        ran.append(case)
        print(f"ok {case}", flush=True)
    torch.cuda.synchronize()
    with open(dst, "w") as fh:
        json.dump(dict(passes=passes, rounds=rounds, cases=ran, forwards=forwards, digit_widths=widths), fh)


if __name__ == "__main__":
    main(sys.argv[1])

"""The binning front end (storage scan, depth sort, rank scan, pair emission, tile sort) with its size-gated variants forced
at small sizes: four depth passes through the 256-bin kernels (GSR_DEPTH_PASSES=4), 4096-element chunks in the pair emission
and the radix passes (GSR_RS_ROUNDS=16), and both.  The knobs are read once per process, so every combination runs in a
child process (tests/binning_child.py), one at a time; the child holds every case to integer-exact references (stable
argsort of the float32 depths, bincount of the pair list, oracle_r's tile lists) and proves through gsr_ctx_info that
each of its forwards took the variant asked for."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 120       # seconds: about thirty forwards of a few thousand Gaussians and one oracle run of 1000 (4 s)
_child_died = []          # a child ended by a signal or at its time limit: nothing more is started on the device


def _expected_cases():
    import test_gpu_binning as G
    return ([f"depth/{d}" for d in G.DEPTH_DISTS + [G.WIDEST]] + [f"live/{v}" for v in G.LIVE_COUNTS]
            + ["tiles-per-rank", "oracle/hydrant-1k"])


@pytest.mark.parametrize("passes,rounds", [(4, None), (None, 16), (4, 16)])
def test_forced_variants_in_a_fresh_process(passes, rounds, tmp_path):
    if _child_died:
        pytest.fail(f"not started: the child for {_child_died[0]} crashed or hung")
    tag = f"GSR_DEPTH_PASSES={passes} GSR_RS_ROUNDS={rounds}"
    env = {k: v for k, v in os.environ.items() if k not in ("GSR_DEPTH_PASSES", "GSR_RS_ROUNDS")}
    if passes:
        env["GSR_DEPTH_PASSES"] = str(passes)
    if rounds:
        env["GSR_RS_ROUNDS"] = str(rounds)
    out = tmp_path / "variants.json"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "binning_child.py"), str(out)], env=env, timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        _child_died.append(tag)
        pytest.fail(f"{tag}: child still running after {CHILD_TIMEOUT} s\n{str(e.stdout)[-3000:]}\n{str(e.stderr)[-3000:]}")
    print(p.stdout[-4000:])
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _child_died.append(tag)
    assert p.returncode == 0, f"{tag}: child failed with status {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    got = json.loads(out.read_text())
    assert got["passes"] == (passes or 3) and got["rounds"] == (rounds or 8)
    assert got["cases"] == _expected_cases()                # a child that silently ran fewer cases fails
    assert got["forwards"] >= len(got["cases"])
    print(f"{tag}: {len(got['cases'])} cases, {got['forwards']} forwards, digit widths {got['digit_widths']}")

"""bench.py as a plain command (`--gpus 1 --steps K --warmup W`): one region of exactly K timed steps, the headline fields
and nothing of what --full adds; --dump-outputs writes what the last timed step computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--P", "20000", "--width", "320", "--height", "192"]


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", *SMALL, *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_times_exactly_steps_and_dumps_reproducible_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--dump-outputs", str(a))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "views/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == 4
    assert len(d["regions_ms"]) == 1                       # one region of exactly --steps steps
    assert abs(d["ms_per_step"] * 4 - d["regions_ms"][0]) <= 0.02 * d["regions_ms"][0] + 0.01
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 0.01
    for k in ("roofline", "stages", "pipelined_streams", "sequential", "batched", "dense", "extras", "pgd", "cpu_baseline",
              "parity"):
        assert k not in d, k
    assert d["config"]["views_per_launch_chain"] == 4
    first = _load(a)
    assert {"render", "radii", "viewspace_grad", "grad_xyz", "grad_features_dc", "grad_features_rest", "grad_opacity",
            "grad_scaling", "grad_rotation"} <= set(first)
    assert first["render"].shape == (4, 3, 320 * 192) and first["grad_features_rest"].shape == (4, 16384, 15, 3)
    assert all(v.dtype == np.float32 for v in first.values())
    assert sum(v.nbytes for v in first.values()) <= 64 << 20
    assert all(np.isfinite(v).all() for v in first.values()) and np.abs(first["grad_xyz"]).max() > 0
    # same arguments, same inputs: output for output the same
    _bench("--dump-outputs", str(b))
    second = _load(b)
    assert set(second) == set(first)
    for k in first:
        assert np.array_equal(first[k], second[k]), k
    # the one-view-per-render() regime ends on the same camera: its last view is the batch's last view
    c = tmp_path / "c"
    d3 = _bench("--headline", "streams", "--dump-outputs", str(c))
    assert d3["config"]["views_per_launch_chain"] == 1 and len(d3["regions_ms"]) == 1
    one = _load(c)
    assert one["render"].shape == (1, 3, 320 * 192)
    assert np.array_equal(one["render"][0], first["render"][-1]) and np.array_equal(one["radii"][0], first["radii"][-1])
    for k in ("viewspace_grad", "grad_xyz", "grad_features_dc", "grad_features_rest", "grad_opacity", "grad_scaling",
              "grad_rotation"):
        ref = first[k][-1]
        np.testing.assert_allclose(one[k][0], ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()), err_msg=k)

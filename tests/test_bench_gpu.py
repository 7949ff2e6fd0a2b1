"""``bench.py``'s contract: a plain run times ``--steps`` steps of the headline loop and nothing else,
``--dump-outputs`` writes the last step's outputs as float32 / float64 ``.npy`` files within 64 MB, and the
same arguments give the same outputs run to run.  (The reference's 89.6 M model: its parameters outnumber
the dump's sample, so the seeded sampling path runs.)"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "grad_norm", "loss_history", "params_sample")
STEPS = 3


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
           "--model", "ref", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


@pytest.fixture(scope="module")
def plain(cuda, tmp_path_factory):
    return _bench(tmp_path_factory.mktemp("bench_a"))


def test_plain_run_result_line_and_dump(plain):
    res, arrs = plain
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, res
    assert res["steps"] == STEPS and res["healthy"] and not res["full"]
    assert "ref_fp32" not in res and "ms_per_step_pipelined" not in res  # --full only
    # value is whole-job tokens/s of the timed loop: batch 8 x 512 tokens per ms_per_step
    assert res["value"] == pytest.approx(8 * 512 / (res["ms_per_step"] / 1e3), rel=1e-3)
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    for name, a in arrs.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert np.isfinite(a).all(), name
    assert arrs["loss_history"].shape == (STEPS,)
    assert float(arrs["loss"]) == arrs["loss_history"][-1]
    assert round(float(arrs["loss"]), 4) == res["config"]["final_loss"]
    assert arrs["params_sample"].ndim == 1 and arrs["params_sample"].size > 0 and arrs["params_sample"].std() > 0


def test_same_arguments_same_outputs(plain, tmp_path):
    _, a = plain
    _, b = _bench(tmp_path)
    assert a["params_sample"].shape == b["params_sample"].shape
    # same tokens, same initial weights, same sampled indices; the kernels' float atomics may reorder sums
    np.testing.assert_allclose(b["loss_history"], a["loss_history"], rtol=1e-4)
    # 5 AdamW steps (2 warmup + 3 timed) at lr 3e-4, |m/sqrt(v)| <= 1, weight decay 0.1 on |p| <= 1: a parameter
    # moves at most 5 * 3e-4 * 1.1 per run, so two runs differ by at most twice that wherever a near-zero
    # gradient changed sign; everywhere else only by the summation order (well under 1e-6)
    d = np.abs(b["params_sample"].astype(np.float64) - a["params_sample"])
    assert d.max() <= 2 * 5 * 3e-4 * 1.1, d.max()
    assert np.median(d) <= 1e-6, np.median(d)

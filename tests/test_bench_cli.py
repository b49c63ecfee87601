"""bench.py's command line on the CPU plumbing path (``--cpu``, one 15625-row block): a plain
run prints the headline line only, ``--full`` adds the secondary figures, and
``--dump-outputs`` writes the last timed step's scores, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--cpu", "--rows", "15625", "--features", "12", "--cv", "3", "--cands-per-rank", "2", "--warmup", "0"]
FULL_ONLY = ("per_rank_fit_ms_per_step", "measured_step_imbalance", "lpt_predicted_imbalance")


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], capture_output=True,
                         text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    plain = _bench("--steps", "2", "--dump-outputs", str(d / "plain"))
    full = _bench("--steps", "1", "--warmup", "1", "--full", "--dump-outputs", str(d / "full"))
    return d, plain, full


def test_plain_run_reports_the_headline_only(runs):
    _d, (rec, err), _full = runs
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec
    assert rec["steps"] == 2 and rec["warmup"] == 0 and rec["unit"] == "CV-fits/s" and rec["higher_is_better"] is True
    fits = rec["steps"] * rec["config"]["global_batch"]
    assert rec["value"] == pytest.approx(fits / (rec["steps"] * rec["ms_per_step"] / 1000.0), rel=1e-3)
    assert not any(k in rec for k in FULL_ONLY) and "phases:" not in err


def test_full_run_adds_the_secondary_figures(runs):
    _d, _plain, (rec, err) = runs
    assert rec["steps"] == 1 and rec["warmup"] == 1
    assert all(k in rec for k in FULL_ONLY) and "phases:" in err
    assert rec["measured_step_imbalance"] == 1.0 and rec["per_rank_fit_ms_per_step"]["max"] > 0


def test_dump_outputs_are_the_last_steps_scores_and_repeat(runs):
    d, (rec, _e), _full = runs
    names = sorted(os.listdir(d / "plain"))
    assert names == sorted(n + ".npy" for n in ("candidate_ids", "cv_scores", "rank0_candidate_ids", "rank0_cv_scores",
                                                "rank0_mean_cv_score", "rank0_std_cv_score"))
    a = {n[:-4]: np.load(d / "plain" / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 1024 * 1024
    assert a["cv_scores"].shape == (2, 3) and a["cv_scores"].dtype == np.float32
    assert np.array_equal(a["candidate_ids"], a["rank0_candidate_ids"])          # one rank: it fits the whole pool
    assert np.array_equal(a["cv_scores"], a["rank0_cv_scores"].astype(np.float32))
    assert np.allclose(a["rank0_mean_cv_score"], a["rank0_cv_scores"].mean(1), rtol=0, atol=1e-12)
    assert rec["mean_cv_accuracy_last_step"] == pytest.approx(float(a["cv_scores"].mean()), abs=1e-4)
    # the other run's only timed step is the same step (index 1) on the same seeded table
    for n in names:
        assert np.array_equal(a[n[:-4]], np.load(d / "full" / n)), n

"""The per-fit score statistics kernel (csrc/kernels/score_stats.hip) against its host twin
(csrc/runtime/score_stats_cpu.cpp) on the same inputs, and a multi-metric job on the GPU data
path against the same job on the CPU data path (docs/MULTIMETRIC.md).

Shapes: F = 7 fits of 0, 1, 63, 64, 65, 257 and (tile + 1) entries -- an empty fit, part of a
wave, a whole wave, more than one wave, more than one pass of the block, and a fit that spans two
blocks with the second cut short -- whose row ids are scattered over a 5,000-row target vector.
Class counts 2, 3, 4 (register counters), 5, 8, 64 (LDS histograms; 4 | 5 is the boundary) and
65 (torch.bincount).

Tolerances: integer counts, and the regression slots whose terms and order of addition are the
same on both sides (0-6, and the invalid-row counts 9, 11, 13), are compared bit for bit.  Slots
7, 8, 10 and 12 divide or take logarithms, where the device's and the host's functions may differ
in the last place: rtol = 1e-12 (their terms are non-negative, so a sum's relative error is at
most its terms').  The figures are printed before they are asserted."""
import json

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.search import scoring
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

N_Y = 5000
EXACT, LOOSE = (0, 1, 2, 3, 4, 5, 6, 9, 11, 13), (7, 8, 10, 12)


def _lens():
    tile = int(native.hip_lib().dml_fit_stats_tile())
    assert tile == int(native.cpu_lib().dml_cpu_fit_stats_tile())
    return (0, 1, 63, 64, 65, 257, tile + 1)


def _case(C, seed):
    rng = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(_lens())]).astype(np.int64)
    rows = rng.randint(0, N_Y, size=off[-1]).astype(np.int32)
    if C:
        y = rng.randint(0, C, size=N_Y).astype(np.int32)
        p = np.where(rng.rand(off[-1]) < 0.6, y[rows], rng.randint(0, C, size=off[-1])).astype(np.int32)
        return off, rows, p, y
    y = (1.0 + rng.normal(size=N_Y)).astype(np.float32)   # some targets below 0 and below -1
    return off, rows, (y[rows] + 0.5 * rng.normal(size=off[-1])).astype(np.float32), y


def _both(off, rows, p, y, C, want=0):
    host = scoring.fit_statistics(torch.from_numpy(rows), off, torch.from_numpy(p), torch.from_numpy(y), C, want=want)
    dev = scoring.fit_statistics(torch.from_numpy(rows).cuda(), off, torch.from_numpy(p).cuda(),
                                 torch.from_numpy(y).cuda(), C, want=want)
    return host, dev


@pytest.mark.parametrize("C", [2, 3, 4, 5, 8, 64, 65])
def test_confusion_matrices_equal_the_twin(C):
    assert int(native.hip_lib().dml_fit_stats_small_c()) == 4 and int(native.hip_lib().dml_fit_stats_max_c()) == 64
    off, rows, p, y = _case(C, 100 + C)
    host, dev = _both(off, rows, p, y, C)
    assert dev.dtype == np.int64 and dev.shape == (7, C, C)
    np.testing.assert_array_equal(dev, host)
    np.testing.assert_array_equal(dev.sum((1, 2)), np.diff(off))
    assert not dev[0].any()                                       # the empty fit has no count ...
    assert C > 8 or (dev[6] > 0).all()                            # ... and the long one fills every cell
    dev2 = scoring.fit_statistics(torch.from_numpy(rows).cuda(), off, torch.from_numpy(p).cuda(),
                                  torch.from_numpy(y).cuda(), C)
    assert dev2.tobytes() == dev.tobytes()                        # two launches, identical bytes
    bad = p.copy()
    bad[off[7] - 1] = C                                           # the one entry of the cut-short block
    bad[off[3] + 2] = -1
    with pytest.raises(ValueError, match=r"fit 3 has 1 prediction"):
        scoring.fit_statistics(torch.from_numpy(rows).cuda(), off, torch.from_numpy(bad).cuda(),
                               torch.from_numpy(y).cuda(), C)


def test_regression_sums_equal_the_twin():
    off, rows, p, y = _case(0, 7)
    host, dev = _both(off, rows, p, y, 0, want=7)
    assert dev.dtype == np.float64 and dev.shape == (7, 14)
    np.testing.assert_array_equal(dev[:, 0], np.diff(off))
    assert dev[6, 9] > 0 and dev[6, 11] > 0 and dev[6, 13] > 0   # every domain check has rows to count
    for j in EXACT:
        assert dev[:, j].tobytes() == host[:, j].tobytes(), (j, dev[:, j], host[:, j])
    for j in LOOSE:
        rel = np.abs(dev[:, j] - host[:, j]) / np.maximum(np.abs(host[:, j]), 1e-300)
        print("slot", j, "max relative difference", rel.max())
        np.testing.assert_allclose(dev[:, j], host[:, j], rtol=1e-12, atol=0)
    host0, dev0 = _both(off, rows, p, y, 0, want=0)
    for j in range(14):   # want clear: the logarithm slots are 0, the others unchanged
        if j in (8, 10, 12):
            assert not dev0[:, j].any() and not host0[:, j].any()
        else:
            assert dev0[:, j].tobytes() == dev[:, j].tobytes()
    dev2 = scoring.fit_statistics(torch.from_numpy(rows).cuda(), off, torch.from_numpy(p).cuda(),
                                  torch.from_numpy(y).cuda(), 0, want=7)
    assert dev2.tobytes() == dev.tobytes()                         # two launches, identical bytes
    for name in ("r2", "neg_root_mean_squared_error", "neg_mean_absolute_error", "explained_variance", "max_error"):
        assert scoring.score_from_stats(name, dev[5]) == scoring.score_from_stats(name, host[5])


def test_job_on_the_gpu_equals_the_cpu_job(tmp_path):
    """LogisticRegression, 300 rows, three metrics, cv=3.  The classes are separated by a margin
    (no row lies near the decision boundary) and 10 % of the labels are flipped, so both data
    paths predict the same labels although their solvers differ in the last places, and the
    confusion matrices are not trivial."""
    import pandas as pd
    from distributed_ml import MLTaskManager
    from sklearn.linear_model import LogisticRegression
    from sklearn.model_selection import GridSearchCV

    from cs230_distributed_machine_learning_amd.config import Config
    from cs230_distributed_machine_learning_amd.engine.service import Controller

    rng = np.random.RandomState(2)
    X = (0.05 * rng.normal(size=(300, 6))).astype(np.float32)
    side = rng.rand(300) < 0.5
    X[:, 0] = np.where(side, 1.0, -1.0) * (0.5 + rng.rand(300))
    y = np.where(rng.rand(300) < 0.1, ~side, side).astype(np.int64)
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(6)])
    df["target"] = y
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    metrics = ["accuracy", "f1_macro", "matthews_corrcoef"]
    outs = {}
    for device in ("cuda", "cpu"):
        c = Controller(Config(data_root=str(tmp_path / f"data_{device}"), device=device, sse_interval_s=0.05))
        try:
            m = MLTaskManager(controller=c)
            assert "error" not in m.download_data(path, "toy", "local")
            est = GridSearchCV(LogisticRegression(max_iter=200), {"C": [0.1, 1.0]}, cv=3, scoring=metrics,
                               refit="f1_macro")
            out = m.train(est, "toy", {"target_column": "target"}, wait_for_completion=True, polling_interval=0.02)
            assert out["job_status"] == "completed", out
            outs[device] = out["job_result"]
        finally:
            c.shutdown()
    key = lambda r: json.dumps(r["parameters"], sort_keys=True)   # noqa: E731
    cpu = {key(r): r for r in outs["cpu"]["results"]}
    for r in outs["cuda"]["results"]:
        assert r["scores"] == cpu[key(r)]["scores"]
        assert 0.8 < r["scores"]["accuracy"]["mean_cv_score"] < 1.0
    assert outs["cuda"]["multimetric"] == outs["cpu"]["multimetric"]

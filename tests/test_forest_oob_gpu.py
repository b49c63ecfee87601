"""The HIP out-of-bag kernels (predict.hip k_oob_cls / k_oob_reg) against their host twin
(csrc/runtime/forest_oob_cpu.cpp) on the same pool: ``out``, ``cnt`` and ``pred`` bit for bit.

Shapes are the smallest that reach each branch: 1000 rows (3 full 256-row blocks + 232) and 100
(one partial block); 13 and 3 trees (no multiple of the lock-step width; with 3 trees some rows
are in every bag); 2 / 3 / 5 / 9 classes (four MAXC instantiations) and regression; 14 features
(rows staged in LDS) and 300 (too wide to stage); trees [13, 16) of the pool read down to depth 3
of 8; a split whose training rows are every third row.  The two environment switches of the
predict launch (read once per process) run in a fresh child process each."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1500
T0, T1 = 13, 3   # fit 0: 13 full trees on split 0; fit 1: 3 trees of depth 8 on split 1


def _specs(d):
    specs = forest_ops.make_specs(T0 + T1)
    for t in range(T0 + T1):
        s = specs[t]
        f = int(t >= T0)
        s["seed"] = 4000 + 17 * t
        s["split"] = f
        s["fit"] = f
        s["max_depth"] = 8 if f else 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = 1
        s["max_features"] = max(1, int(np.sqrt(d)))
        s["bootstrap"] = 1
        s["criterion"] = 0
        s["pois_cdf"] = native.poisson_cdf_table(1.0)
    return specs


def _table(C, d):
    """C >= 2 classes, or C == 0: regression.  uint8 bins, a target that depends on them."""
    rng = np.random.RandomState(100 * C + d)
    Xb = rng.randint(0, 32, size=(N, d)).astype(np.uint8)
    z = Xb[:, 0].astype(np.float64) + 0.5 * Xb[:, 1] - 0.7 * Xb[:, d - 1] + rng.normal(0, 4, N)
    roles = np.full((2, N), 2, np.uint8)
    roles[0, np.sort(rng.permutation(N)[:1000])] = 1
    roles[1, ::3] = 1                                  # every third row
    if C:
        q = np.quantile(z, np.linspace(0, 1, C + 1)[1:-1])
        return Xb, np.searchsorted(q, z).astype(np.int32), None, roles
    return Xb, None, z.astype(np.float32), roles


def compare_pool(C, d):
    """Build one pool on the GPU, copy it to the host, and compare the two OOB walks on it."""
    dev = torch.device("cuda:0")
    Xb_cpu, ycls, yreg, roles = _table(C, d)
    is_reg = C == 0
    specs = _specs(d)
    if is_reg:
        specs["criterion"] = forest_ops.MSE
    pitch = (d + 3) // 4 * 4                           # whole dwords per row: the staged path's layout
    buf = torch.zeros((N, pitch), dtype=torch.uint8, device=dev)
    buf[:, :d] = torch.from_numpy(Xb_cpu).to(dev)
    Xb = buf[:, :d]
    g = forest_ops.build_gpu(Xb, None if is_reg else torch.from_numpy(ycls).to(dev),
                             None if not is_reg else torch.from_numpy(yreg).to(dev),
                             torch.from_numpy(roles).to(dev), specs, max(C, 1), is_reg)
    torch.cuda.synchronize(dev)
    c = g.to_numpy()
    rows0 = np.nonzero(roles[0] == 1)[0].astype(np.int32)
    rows1 = np.nonzero(roles[1] == 1)[0].astype(np.int32)
    assert len(rows0) == 1000 and len(rows1) == 500
    seen_empty = False
    for t0, t1, rows, cap in ((0, T0, rows0, 0), (0, T0, rows0[:100], 0), (T0, T0 + T1, rows1, 3),
                              (T0, T0 + T1, rows1, 0)):
        got = forest_ops.oob_predict(g, Xb, specs, t0, t1, torch.from_numpy(rows).to(dev), depth_cap=cap)
        ref = forest_ops.oob_predict(c, Xb_cpu, specs, t0, t1, rows, depth_cap=cap)
        assert len(got) == len(ref) == (2 if is_reg else 3)
        for a, b in zip(got, ref):
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and a.shape == b.shape
            assert np.array_equal(a, b), (C, d, t0, t1, cap, int((a != b).sum()))
        cnt = ref[1]
        assert cnt.max() <= t1 - t0 and cnt.sum() > 0.25 * len(rows) * (t1 - t0)
        if (cnt == 0).any():
            seen_empty = True
            assert not np.any(ref[0][cnt == 0])
        if cap:   # the cap is read: depth 3 of 8 gives other leaves than the whole trees
            whole = forest_ops.oob_predict(c, Xb_cpu, specs, t0, t1, rows)
            assert not np.array_equal(whole[0], ref[0])
    assert seen_empty   # 3 trees: 0.632^3 of the rows are in every bag
    return True


@pytest.mark.parametrize("C,d", [(2, 14), (3, 14), (5, 14), (9, 14), (0, 14), (3, 300), (0, 300)])
def test_oob_kernel_is_bit_equal_to_host_twin(C, d):
    assert compare_pool(C, d)


@pytest.mark.parametrize("switch", ["DML_PRED_NO_STAGE", "DML_PRED_NO_TOP"])
def test_oob_kernel_under_predict_switches(switch):
    """No LDS row staging / no LDS top table: read once per process, so a fresh child runs them."""
    env = dict(os.environ, **{switch: "1"})
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "5", "14"], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "oob pools equal" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("is_cls", [True, False])
def test_job_oob_score_is_the_cpu_jobs(is_cls):
    """End to end on the device: the trees are bit-identical across builders, so the job's
    oob_score is the CPU job's; and asking for it leaves the CV scores alone.  Candidate 1 is a
    depth-capped prefix of candidate 0 on the device and a fit of its own on the CPU."""
    from sklearn.datasets import make_classification, make_regression

    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates

    name = "RandomForestClassifier" if is_cls else "RandomForestRegressor"
    if is_cls:
        X, y = make_classification(400, 8, n_informative=5, n_classes=3, random_state=8)
    else:
        X, y = make_regression(400, 8, n_informative=5, noise=5, random_state=8)
    X = X.astype(np.float32)

    def job(device, flag):
        cands = [{"n_estimators": 20, "max_depth": 6, "oob_score": flag, "random_state": 0},
                 {"n_estimators": 10, "max_depth": 3, "oob_score": flag, "random_state": 0}]
        res = run_candidates(DeviceData(X, y, is_cls, device), JobSpec(name, cands, cv=2, holdout=True), range(2))
        assert all(r.ok for r in res), [r.error for r in res]
        return res

    gpu, cpu, plain = job("cuda:0", True), job("cpu", True), job("cuda:0", False)
    key = "oob_decision_function" if is_cls else "oob_prediction"
    for g, c, p in zip(gpu, cpu, plain):
        assert abs(g.result["oob_score"] - c.result["oob_score"]) <= 1e-12
        assert g.result["oob_score"] == g.model["oob_score"]
        np.testing.assert_array_equal(g.model[key], c.model[key])
        np.testing.assert_array_equal(g.model["oob_rows"], c.model["oob_rows"])
        np.testing.assert_allclose(g.model["feature_importances"], c.model["feature_importances"], rtol=0, atol=1e-12)
        assert g.result["cv_scores"] == p.result["cv_scores"]
        assert "oob_score" not in p.result and key not in p.model
    assert gpu[0].result["oob_score"] != gpu[1].result["oob_score"]


if __name__ == "__main__":   # the child of test_oob_kernel_under_predict_switches
    ok = compare_pool(int(sys.argv[1]), int(sys.argv[2]))
    print("oob pools equal" if ok else "differ")

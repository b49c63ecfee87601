"""The HIP permutation-importance kernels (predict.hip k_perm_cls / k_perm_reg / k_perm_reduce)
against their host twin (csrc/runtime/forest_perm_cpu.cpp) on the same pool: the permuted
predictions bit for bit, the match counts equal, the squared-error sums to rel 1e-12 (the kernel
adds a block's rows by lane shuffles, the twin in row order).

Shapes are the smallest that reach each branch: 300 rows (one full 256-row block and a partly
live one) and 257 (one row past the block boundary); 6 features (rows staged in LDS) and 260
(too wide to stage: the substituted bin exists only in the compare); 2 and 3 classes and
regression; 11 trees after 3 trees of another fit (a mid-pool range whose last lock-step group of
8 is partial), 5 trees for the wide table; 1 and 5 repeats; whole trees and a depth cap of 3; the
last feature is constant, so no tree splits on it."""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

N = 800
T_FIRST = 3


def _specs(T, d, is_reg):
    specs = forest_ops.make_specs(T_FIRST + T)
    for t in range(T_FIRST + T):
        s = specs[t]
        s["seed"] = 900 + 31 * t
        s["split"] = 0
        s["fit"] = int(t >= T_FIRST)
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = 1
        s["max_features"] = max(1, int(np.sqrt(d)))
        s["bootstrap"] = 1
        s["criterion"] = forest_ops.MSE if is_reg else 0
        s["pois_cdf"] = native.poisson_cdf_table(1.0)
    return specs


def _table(C, d, n_rows):
    """C >= 2 classes, or C == 0: regression.  uint8 bins, the last column constant; 400 training
    rows and ``n_rows`` held-out ones."""
    rng = np.random.RandomState(10 * C + d + n_rows)
    Xb = rng.randint(0, 32, size=(N, d)).astype(np.uint8)
    Xb[:, d - 1] = 7
    z = Xb[:, 0].astype(np.float64) + 0.5 * Xb[:, 1] - 0.7 * Xb[:, d - 2] + rng.normal(0, 3, N)
    order = rng.permutation(N)
    roles = np.zeros((1, N), np.uint8)
    roles[0, order[:400]] = 1
    roles[0, order[400:400 + n_rows]] = 2
    if C:
        q = np.quantile(z, np.linspace(0, 1, C + 1)[1:-1])
        return Xb, np.searchsorted(q, z).astype(np.int32), None, roles
    return Xb, None, z.astype(np.float32), roles


@pytest.mark.parametrize("C,d,n_rows,T,K,cap", [
    (2, 6, 300, 11, 5, 0), (3, 6, 257, 11, 1, 0), (3, 6, 300, 11, 5, 3), (0, 6, 300, 11, 5, 0),
    (0, 6, 257, 11, 1, 3), (3, 260, 300, 5, 5, 0), (0, 260, 300, 5, 1, 0)])
def test_perm_kernel_equals_host_twin(C, d, n_rows, T, K, cap):
    dev = torch.device("cuda:0")
    is_reg = C == 0
    Xb_cpu, ycls, yreg, roles = _table(C, d, n_rows)
    specs = _specs(T, d, is_reg)
    pitch = (d + 3) // 4 * 4                           # whole dwords per row: the staged path's layout
    buf = torch.zeros((N, pitch), dtype=torch.uint8, device=dev)
    buf[:, :d] = torch.from_numpy(Xb_cpu).to(dev)
    Xb = buf[:, :d]
    y_dev = torch.from_numpy(yreg if is_reg else ycls).to(dev)
    g = forest_ops.build_gpu(Xb, None if is_reg else y_dev, y_dev if is_reg else None,
                             torch.from_numpy(roles).to(dev), specs, max(C, 1), is_reg)
    torch.cuda.synchronize(dev)
    c = g.to_numpy()
    rows = np.nonzero(roles[0] == 2)[0].astype(np.int32)
    assert len(rows) == n_rows
    perm = forest_ops.permutation_indices(n_rows, K, 3)
    t0, t1 = T_FIRST, T_FIRST + T
    kw = dict(depth_cap=cap, want_pred=True, want_walked=True)
    got = forest_ops.permutation_scores(g, Xb, t0, t1, torch.from_numpy(rows).to(dev), perm,
                                        ycls=None if is_reg else y_dev, yreg=y_dev if is_reg else None, **kw)
    ref = forest_ops.permutation_scores(c, Xb_cpu, t0, t1, rows, perm, ycls=ycls, yreg=yreg, **kw)
    assert got["sums"].is_cuda and got["pred"].is_cuda
    np.testing.assert_array_equal(got["features"], ref["features"])
    assert d - 1 not in ref["features"] and len(ref["features"]) >= min(d - 1, 4)
    for key in ("pred", "base_pred", "walked"):
        a, b = got[key].cpu().numpy(), ref[key].numpy()
        assert a.dtype == b.dtype and a.shape == b.shape
        assert np.array_equal(a, b), (key, int((a != b).sum()))
    gs, rs = got["sums"].cpu().numpy(), ref["sums"].numpy()
    assert gs.shape == rs.shape == (d, K) and gs.dtype == rs.dtype
    gb, rb = got["base"].cpu().numpy(), ref["base"].numpy()
    print("sums: max rel diff", np.abs(gs - rs).max() / max(np.abs(rs).max(), 1), "base", gb, rb)
    if is_reg:
        np.testing.assert_allclose(gs, rs, rtol=1e-12, atol=0)
        np.testing.assert_allclose(gb, rb, rtol=1e-12, atol=0)
        assert abs(got["ss_tot"] - ref["ss_tot"]) <= 1e-12 * ref["ss_tot"]
    else:
        np.testing.assert_array_equal(gs, rs)
        np.testing.assert_array_equal(gb, rb)
    # the unused feature's statistics are the baseline's, and the walk changes something elsewhere
    assert np.all(rs[d - 1] == rb[0]) and not np.all(rs[:2] == rb[0])
    assert ref["walked"].sum() > 0 and ref["walked"][d - 1] == 0
    if cap:   # the cap is read: other predictions than the whole trees give
        whole = forest_ops.permutation_scores(c, Xb_cpu, t0, t1, rows, perm, ycls=ycls, yreg=yreg, want_pred=True)
        assert not np.array_equal(whole["pred"].numpy(), ref["pred"].numpy())
    # determinism: a second run gives the same sums, bit for bit
    again = forest_ops.permutation_scores(g, Xb, t0, t1, torch.from_numpy(rows).to(dev), perm,
                                          ycls=None if is_reg else y_dev, yreg=y_dev if is_reg else None,
                                          depth_cap=cap)
    assert torch.equal(again["sums"], got["sums"]) and torch.equal(again["base"], got["base"])


@pytest.mark.parametrize("is_cls", [True, False])
def test_job_permutation_importance_is_the_cpu_jobs(is_cls):
    """End to end on the device: the trees are bit-identical across builders, so the job's
    importances are the CPU job's -- equal for accuracy; for r2 each score is 1 - SSE / ss_tot with
    SSE within rel 1e-12 and SSE / ss_tot below 2, so within 4e-12.  Candidate 1 is a depth-capped
    prefix of candidate 0 on the device and a fit of its own on the CPU."""
    from sklearn.datasets import make_classification, make_regression

    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates

    name = "RandomForestClassifier" if is_cls else "RandomForestRegressor"
    if is_cls:
        X, y = make_classification(400, 8, n_informative=5, n_classes=3, random_state=8)
    else:
        X, y = make_regression(400, 8, n_informative=5, noise=5, random_state=8)
    X = X.astype(np.float32)
    opts = {"n_repeats": 3, "random_state": 2, "scoring": "accuracy" if is_cls else "r2", "candidates": "all"}

    def job(device, perm):
        cands = [{"n_estimators": 20, "max_depth": 6, "random_state": 0},
                 {"n_estimators": 10, "max_depth": 3, "random_state": 0}]
        res = run_candidates(DeviceData(X, y, is_cls, device),
                             JobSpec(name, cands, cv=2, holdout=True, permutation=perm), range(2))
        assert all(r.ok for r in res), [r.error for r in res]
        return res

    gpu, cpu, plain = job("cuda:0", opts), job("cpu", opts), job("cuda:0", None)
    for g, c, p in zip(gpu, cpu, plain):
        ge, ce = g.result["permutation_importance"], c.result["permutation_importance"]
        np.testing.assert_array_equal(g.model["permutation_rows"], c.model["permutation_rows"])
        if is_cls:
            np.testing.assert_array_equal(g.model["permutation_importances"], c.model["permutation_importances"])
            # the reported baseline is the job's own holdout accuracy: torch's mean of n zeros and ones
            # in double, whose rounding depends on the device's reduction (each step within 2^-53)
            assert ge["baseline_score"] == g.result["accuracy"] and ce["baseline_score"] == c.result["accuracy"]
            assert abs(ge["baseline_score"] - ce["baseline_score"]) <= len(g.model["permutation_rows"]) * 2.0**-53
            assert {k: v for k, v in ge.items() if k != "baseline_score"} == \
                {k: v for k, v in ce.items() if k != "baseline_score"}
        else:
            np.testing.assert_allclose(g.model["permutation_importances"], c.model["permutation_importances"],
                                       rtol=0, atol=4e-12)
            assert abs(ge["baseline_score"] - ce["baseline_score"]) <= 4e-12
            assert ge["baseline_score"] == g.result["r2_score"]
        assert max(ge["importances_mean"]) > 0.02
        assert g.result["cv_scores"] == p.result["cv_scores"]
        assert "permutation_importance" not in p.result
    assert gpu[0].result["permutation_importance"] != gpu[1].result["permutation_importance"]

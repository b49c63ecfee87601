"""The HIP partial-dependence kernels (predict.hip k_pd_cls / k_pd_reg / k_pd_reduce) against their
host twin (csrc/runtime/forest_pd_cpu.cpp) on the same pool: the per-row values bit for bit, the
count of slots walked a second time equal, the averages to rel 1e-12 (the twin adds a block's
rows in the kernel's own order, so they are in fact equal; the bound is the order of one float64
sum of n <= 300 float32 values).

Shapes are the smallest that reach each branch: 300 rows (one full 256-row block and a partly live
one) and 257 (one row past the block boundary); 6 features (rows staged in LDS) and 260 (too wide
to stage: the substituted bin exists only in the compare); 2, 3 and 5 classes (5: accumulator
chunks of 4 grid points) and regression; 11 trees after 3 trees of another fit (a mid-pool range
whose last lock-step group of 8 is partial), 5 trees for the wide table; 1 and 9 grid points (9:
one full chunk of 8 and one more); whole trees and a depth cap of 3; the last feature is constant,
so no tree splits on it; feature 0's bin list holds one bin twice and the bin most rows have."""
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
    rows and ``n_rows`` rows to average over."""
    rng = np.random.RandomState(10 * C + d + n_rows)
    Xb = rng.randint(0, 32, size=(N, d)).astype(np.uint8)
    Xb[:, d - 1] = 7
    Xb[rng.uniform(size=N) < 0.4, 0] = 12            # many rows share feature 0's bin 12
    z = Xb[:, 0].astype(np.float64) + 0.5 * Xb[:, 1] - 0.7 * Xb[:, d - 2] + rng.normal(0, 3, N)
    order = rng.permutation(N)
    roles = np.zeros((1, N), np.uint8)
    roles[0, order[:400]] = 1
    roles[0, order[400:400 + n_rows]] = 2
    if C:
        q = np.quantile(z, np.linspace(0, 1, C + 1)[1:-1])
        return Xb, np.searchsorted(q, z).astype(np.int32), None, roles
    return Xb, None, z.astype(np.float32), roles


def _bins(d, G):
    """Features 0, 1, d - 2 (informative) and d - 1 (unused), G bins each; with G = 9 feature 0's
    list holds bin 3 twice and bin 12, the own bin of many rows."""
    feats = [0, 1, d - 2, d - 1]
    rng = np.random.RandomState(G)
    sub = np.stack([rng.choice(40, G, replace=False) for _ in feats]).astype(np.uint8)
    if G >= 3:
        sub[0, :3] = (3, 12, 3)
    return feats, sub, [G] * len(feats)


@pytest.mark.parametrize("C,d,n_rows,T,G,cap", [
    (2, 6, 300, 11, 9, 0), (3, 6, 257, 11, 1, 0), (3, 6, 300, 11, 9, 3), (5, 6, 257, 11, 9, 0),
    (0, 6, 300, 11, 9, 0), (0, 6, 257, 11, 1, 3), (3, 260, 300, 5, 9, 0), (0, 260, 300, 5, 1, 0)])
def test_pd_kernel_equals_host_twin(C, d, n_rows, T, G, cap):
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
    feats, sub, ng = _bins(d, G)
    NT = 1 if C in (0, 2) else C
    t0, t1 = T_FIRST, T_FIRST + T
    kw = dict(depth_cap=cap, want_rows=True, want_walked=True)
    rows_dev = torch.from_numpy(rows).to(dev)
    got = forest_ops.partial_dependence_values(g, Xb, t0, t1, rows_dev, feats, sub, ng, **kw)
    ref = forest_ops.partial_dependence_values(c, Xb_cpu, t0, t1, rows, feats, sub, ng, **kw)
    assert got["rows"].is_cuda
    np.testing.assert_array_equal(got["features"], ref["features"])
    assert list(ref["features"]) == feats[:3]                        # the constant column is not walked
    for key in ("rows", "base_rows"):
        a, b = got[key].cpu().numpy(), ref[key].numpy()
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
        assert np.array_equal(a, b), (key, int((a != b).sum()))
    assert got["rows"].shape == (4, G, n_rows, NT)
    np.testing.assert_array_equal(got["walked"], ref["walked"])
    assert got["base_walked"] == ref["base_walked"] == 0
    ga, ra = got["average"], ref["average"]
    assert ga.shape == ra.shape == (4, G, NT) and ga.dtype == ra.dtype == np.float64
    print("average: max rel diff", (np.abs(ga - ra) / np.abs(ra)).max(), "equal", np.array_equal(ga, ra))
    np.testing.assert_allclose(ga, ra, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["baseline"], ref["baseline"], rtol=1e-12, atol=0)
    # the averages are the float64 means of the per-row values
    np.testing.assert_allclose(ra, ref["rows"].numpy().astype(np.float64).mean(2), rtol=1e-12, atol=0)
    # the unused feature equals the baseline at every grid point; the walk changes something elsewhere
    assert np.all(ga[3] == got["baseline"]) and np.all(ra[3] == ref["baseline"])
    assert ref["walked"][3] == 0 and ref["walked"][:3].min() > 0
    assert not np.all(ra[0] == ref["baseline"])
    if G >= 3:   # the duplicate bin: walked once, its values copied
        assert np.array_equal(got["rows"][0, 0].cpu().numpy(), got["rows"][0, 2].cpu().numpy())
        assert np.array_equal(ga[0, 0], ga[0, 2])
    # the kernel against itself: no_skip walks every tree for every grid point, to the same values
    ns = forest_ops.partial_dependence_values(g, Xb, t0, t1, rows_dev, feats, sub, ng, no_skip=True, **kw)
    assert torch.equal(ns["rows"], got["rows"])
    assert np.all(ns["walked"][:3] > got["walked"][:3])
    ns_ref = forest_ops.partial_dependence_values(c, Xb_cpu, t0, t1, rows, feats, sub, ng, no_skip=True, **kw)
    np.testing.assert_array_equal(ns["walked"], ns_ref["walked"])
    if cap:   # the cap is read: other values than the whole trees give
        whole = forest_ops.partial_dependence_values(g, Xb, t0, t1, rows_dev, feats, sub, ng, want_rows=True)
        assert not torch.equal(whole["rows"], got["rows"])
    # determinism: a second run gives the same averages, bit for bit
    again = forest_ops.partial_dependence_values(g, Xb, t0, t1, rows_dev, feats, sub, ng, depth_cap=cap)
    assert np.array_equal(again["average"], ga) and np.array_equal(again["baseline"], got["baseline"])


@pytest.mark.parametrize("is_cls", [True, False])
def test_job_partial_dependence_is_the_cpu_jobs(is_cls):
    """End to end on the device: the refit's trees are bit-identical across builders, so its
    partial dependence is the CPU job's (rel 1e-12: the order of one float64 sum)."""
    from sklearn.datasets import make_classification, make_regression

    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import partial_dependence_entry
    from cs230_distributed_machine_learning_amd.engine.service import job_plan, refit_model

    name = "RandomForestClassifier" if is_cls else "RandomForestRegressor"
    if is_cls:
        X, y = make_classification(400, 8, n_informative=5, n_classes=3, random_state=8)
    else:
        X, y = make_regression(400, 8, n_informative=5, noise=5, random_state=8)
    X = X.astype(np.float32)
    params = {"n_estimators": 20, "max_depth": 6, "random_state": 0}
    plan = job_plan({"model_details": {"model_type": name, "hyperparameters": params},
                     "train_params": {"partial_dependence": {"grid_resolution": 10, "max_rows": 300, "random_state": 1}}})

    def job(device):
        model = refit_model(plan, params, DeviceData(X, y, is_cls, device))
        assert model is not None
        return model, partial_dependence_entry(model)

    (gm, ge), (cm, ce) = job("cuda:0"), job("cpu")
    np.testing.assert_array_equal(gm["nodes"], cm["nodes"])
    np.testing.assert_array_equal(gm["pd_rows"], cm["pd_rows"])
    np.testing.assert_array_equal(gm["pd_grid_values"], cm["pd_grid_values"])
    assert gm["pd_average"].shape == cm["pd_average"].shape == (3 if is_cls else 1, 80)
    print("job average: max rel diff", (np.abs(gm["pd_average"] - cm["pd_average"]) / np.abs(cm["pd_average"])).max())
    np.testing.assert_allclose(gm["pd_average"], cm["pd_average"], rtol=1e-12, atol=0)
    assert {k: v for k, v in ge.items() if k != "average"} == {k: v for k, v in ce.items() if k != "average"}
    assert np.ptp(gm["pd_average"], axis=1).max() > (0.02 if is_cls else 1.0)

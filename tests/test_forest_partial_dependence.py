"""One-way partial dependence of kept RandomForest* models (docs/PARTIAL_DEPENDENCE.md): the grids
against ``sklearn.inspection.partial_dependence`` itself, the host walk
(csrc/runtime/forest_pd_cpu.cpp) against the artefact's own ``Predictor`` with the column
overwritten, and the plumbing from ``train_params`` to the result, the artefact and
``Predictor.partial_dependence``.

Shapes: 500 rows and 4 features for the grids (continuous, 7-valued, exactly ``grid_resolution``
values, constant); 300 rows and 6 features for the jobs (2 informative, feature 3 with 5 values,
feature 5 constant: no tree can split on it), 7 trees, a grid of 6, 200 of the 300 rows."""
import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.model_store import load_model
from cs230_distributed_machine_learning_amd.engine.service import Controller, job_plan, refit_model
from cs230_distributed_machine_learning_amd.models.base import FitTask, ParamError, family_of
from cs230_distributed_machine_learning_amd.ops import forest_ops

sk = pytest.importorskip("sklearn")
from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor  # noqa: E402
from sklearn.inspection import partial_dependence as sk_partial_dependence  # noqa: E402
from sklearn.model_selection import GridSearchCV  # noqa: E402

CLS, REG = "RandomForestClassifier", "RandomForestRegressor"
N, D, G, MAX_ROWS, SEED = 300, 6, 6, 200, 11
PD_KEYS = ("pd_features", "pd_grid_off", "pd_grid_values", "pd_average", "pd_rows", "pd_meta")
OPTS = {"grid_resolution": G, "max_rows": MAX_ROWS, "random_state": SEED}


# ---- the grids -------------------------------------------------------------------------------
def _grid_table():
    rng = np.random.RandomState(2)
    X = np.empty((500, 4), dtype=np.float32)
    X[:, 0] = rng.normal(size=500)
    X[:, 1] = rng.randint(0, 7, 500)
    X[:, 2] = np.arange(500) % 20            # exactly grid_resolution distinct values: not "fewer than"
    X[:, 3] = 1.5
    return X, (X[:, 0] > 0).astype(np.int64)


@pytest.fixture(scope="module")
def sk_rf():
    X, y = _grid_table()
    return RandomForestClassifier(n_estimators=3, random_state=0).fit(X, y)


@pytest.mark.parametrize("percentiles", [(0.05, 0.95), (0.1, 0.6)])
@pytest.mark.parametrize("f", [0, 1, 2, 3])
def test_grid_is_sklearns(sk_rf, f, percentiles):
    X, _y = _grid_table()
    ref = sk_partial_dependence(sk_rf, X, [f], method="brute", grid_resolution=20, percentiles=percentiles)
    got = forest_ops.partial_dependence_grid(X[:, f], 20, percentiles)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, np.asarray(ref["grid_values"][0], dtype=np.float64))
    assert len(got) == (20, 7, 20, 1)[f]


def test_grid_percentiles_too_close():
    col = np.zeros(500, dtype=np.float32)
    col[:30] = np.arange(30)                  # 30 distinct values, but both percentiles sit on the zeros
    assert forest_ops.partial_dependence_grid(col, 20, (0.2, 0.8)) is None
    with pytest.raises(ValueError, match="percentiles are too close"):
        sk_partial_dependence(RandomForestRegressor(n_estimators=1).fit(col.reshape(-1, 1), col), col.reshape(-1, 1), [0],
                              method="brute", grid_resolution=20, percentiles=(0.2, 0.8))


# ---- values: the host twin through a job -----------------------------------------------------
def _table(kind):
    """kind: 2 / 3 classes, or 0: regression."""
    rng = np.random.RandomState(5)
    X = rng.normal(size=(N, D)).astype(np.float32)
    X[:, 3] = rng.randint(0, 5, N)
    X[:, 5] = 1.0
    z = 2.0 * X[:, 0] - X[:, 1] + 0.4 * X[:, 3] + 0.1 * rng.normal(size=N)
    if kind:
        return X, np.searchsorted(np.quantile(z, np.linspace(0, 1, kind + 1)[1:-1]), z).astype(np.int64)
    return X, z.astype(np.float32)


@pytest.fixture
def ctl(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), journal=str(tmp_path / "journal.jsonl"), device="cpu",
                          sse_interval_s=0.05))
    yield c
    c.shutdown()


def _client(ctl, tmp_path, kind):
    import pandas as pd
    from distributed_ml import MLTaskManager

    X, y = _table(kind)
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D)])
    df["target"] = y
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    m = MLTaskManager(controller=ctl)
    assert "error" not in m.download_data(path, "toy", "local")
    return m, X


def _train(m, est, option, **extra):
    tp = {"target_column": "target", **extra}
    if option is not None:
        tp["partial_dependence"] = option
    return m.train(est, "toy", tp, wait_for_completion=True, polling_interval=0.02)


def _check_against_predictor(est, X, kind):
    """``average`` of every computed feature and grid value against the artefact's own predictions
    of the rows with the column overwritten; returns the largest relative difference."""
    raw = est.model
    rows = np.asarray(raw["pd_rows"])
    worst = 0.0
    for f in [int(v) for v in raw["pd_features"]]:
        pdp = est.partial_dependence(f)
        n_targets = kind if kind > 2 else 1
        assert pdp.average.shape == (n_targets, len(pdp.grid_values[0])) and pdp.average.dtype == np.float64
        for g, v in enumerate(pdp.grid_values[0]):
            Xe = X[rows].copy()
            Xe[:, f] = v
            if kind:
                ref = est.predict_proba(Xe).mean(0)
                ref = ref[1:] if kind == 2 else ref          # binary: the positive class only, as sklearn
            else:
                ref = np.array([est.predict(Xe).astype(np.float64).mean()])
            np.testing.assert_allclose(pdp.average[:, g], ref, rtol=1e-12, atol=0)
            worst = max(worst, float((np.abs(pdp.average[:, g] - ref) / np.abs(ref)).max()))
    return worst


@pytest.mark.parametrize("kind", [2, 3, 0])
def test_job_values_are_the_artefacts_predictions(ctl, tmp_path, kind):
    from distributed_ml import MLTaskManager

    m, X = _client(ctl, tmp_path, kind)
    base = RandomForestClassifier(n_estimators=7) if kind else RandomForestRegressor(n_estimators=7)
    out = _train(m, GridSearchCV(base, {"max_depth": [3, None]}, cv=2), OPTS)
    assert out["job_status"] == "completed", out
    path = m.download_best_model(dest=str(tmp_path / "best.npz"))
    est = MLTaskManager.load_model(path)
    raw = est.model
    # the refit model's training rows are every row; more than max_rows, so the stated subsample
    rows = np.arange(N)[np.sort(np.random.RandomState(SEED).choice(N, MAX_ROWS, replace=False))]
    np.testing.assert_array_equal(raw["pd_rows"], rows)
    assert raw["pd_rows"].dtype == np.int32 and raw["pd_features"].dtype == np.int32
    assert raw["pd_grid_off"].dtype == np.int64 and raw["pd_grid_values"].dtype == np.float64
    np.testing.assert_array_equal(raw["pd_features"], np.arange(D))
    np.testing.assert_array_equal(np.diff(raw["pd_grid_off"]), [G, G, G, 5, G, 1])
    for f in range(D):   # the grids are sklearn's on those rows
        np.testing.assert_array_equal(est.partial_dependence(f).grid_values[0],
                                      forest_ops.partial_dependence_grid(X[rows, f], G, (0.05, 0.95)))
    print("kind", kind, "max rel |average - predictor mean| =", _check_against_predictor(est, X, kind))
    # the constant column: one grid point, and (no tree splits on it) the baseline mean
    const = est.partial_dependence(5)
    base_mean = est.predict_proba(X[rows]).mean(0) if kind else np.array([est.predict(X[rows]).astype(np.float64).mean()])
    base_mean = base_mean[1:] if kind == 2 else base_mean
    assert const.average.shape[1] == 1
    np.testing.assert_allclose(const.average[:, 0], base_mean, rtol=1e-12, atol=0)
    assert np.ptp(est.partial_dependence(0).average, axis=1).max() > 0.1     # an informative one moves
    # the result entry is the artefact's arrays
    entry = out["best_result"]["partial_dependence"]
    assert entry["features"] == list(range(D)) and entry["n_rows"] == MAX_ROWS
    assert (entry["grid_resolution"], entry["percentiles"], entry["max_rows"], entry["random_state"]) == \
        (G, [0.05, 0.95], MAX_ROWS, SEED)
    off = raw["pd_grid_off"]
    for j in range(D):
        assert entry["grid_values"][j] == raw["pd_grid_values"][off[j]:off[j + 1]].tolist()
        assert entry["average"][j] == raw["pd_average"][:, off[j]:off[j + 1]].tolist()
    others = [r for r in out["job_result"]["results"] if r["parameters"] != out["best_result"]["parameters"]]
    assert others and all("partial_dependence" not in r for r in others)
    # the accessor: by name too, and its two errors
    by_name = est.partial_dependence("f3")
    np.testing.assert_array_equal(by_name.average, est.partial_dependence(3).average)
    assert by_name.feature == 3 and by_name.n_rows == MAX_ROWS
    with pytest.raises(KeyError):
        est.partial_dependence(D)
    with pytest.raises(KeyError):
        est.partial_dependence("nope")


def test_features_option_and_uncomputed_feature(ctl, tmp_path):
    m, X = _client(ctl, tmp_path, 3)
    out = _train(m, RandomForestClassifier(n_estimators=5, random_state=0), {**OPTS, "features": [4, 0], "max_rows": None})
    assert out["job_status"] == "completed", out
    est = m.download_best_model(dest=str(tmp_path / "best.npz"), load=True)
    np.testing.assert_array_equal(est.model["pd_features"], [4, 0])
    np.testing.assert_array_equal(est.model["pd_rows"], np.arange(N))       # max_rows=None: every row
    entry = out["job_result"]["results"][0]["partial_dependence"]      # a plain fit job: one result
    assert entry["features"] == [4, 0] and entry["max_rows"] is None and entry["n_rows"] == N
    _check_against_predictor(est, X, 3)
    with pytest.raises(KeyError, match="not computed"):
        est.partial_dependence(1)


def test_depth_capped_winner_gets_its_own_values(ctl, tmp_path):
    """One threshold on feature 0 with a quarter of the labels flipped: the stump forest
    (max_depth=1, a depth prefix of the deep candidate where prefixes are shared) cannot fit the
    flips and wins the search; its values are those of its own, shallow artefact."""
    import pandas as pd
    from distributed_ml import MLTaskManager

    rng = np.random.RandomState(3)
    X = rng.normal(size=(N, D)).astype(np.float32)
    y = ((X[:, 0] > 0) ^ (rng.uniform(size=N) < 0.25)).astype(np.int64)
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D)])
    df["target"] = y
    df.to_csv(str(tmp_path / "noise.csv"), index=False)
    m = MLTaskManager(controller=ctl)
    assert "error" not in m.download_data(str(tmp_path / "noise.csv"), "toy", "local")
    out = _train(m, GridSearchCV(RandomForestClassifier(n_estimators=9, random_state=4), {"max_depth": [None, 1]}, cv=3),
                 OPTS)
    assert out["job_status"] == "completed", out
    assert out["best_result"]["parameters"]["max_depth"] == 1, out["best_result"]
    est = m.download_best_model(dest=str(tmp_path / "best.npz"), load=True)
    assert int((np.asarray(est.model["nodes"])[:, 0] >= 0).sum()) <= 9        # stumps: one split per tree
    _check_against_predictor(est, X, 2)


def test_prefix_follower_walks_its_own_trees_and_cap():
    """A follower task (the leader's first trees, read down to its own depth) gets the values of its
    own artefact: ``_attach_pd`` passes the tree range and the depth cap."""
    from cs230_distributed_machine_learning_amd.engine.model_store import Predictor, _forest_build
    from cs230_distributed_machine_learning_amd.models.forest import extract_forest

    X, y = _table(3)
    dd = DeviceData(X, y, True, "cpu")
    roles = np.ones((1, N), np.uint8)
    dd.set_splits(roles, ["full"])
    fam = family_of(CLS)
    tasks = [FitTask(i, i, 0, CLS, fam.resolve(CLS, {"n_estimators": T, "random_state": 5 + i}, N, D, dd.n_classes))
             for i, T in enumerate((2, 7))]
    specs = fam._specs(tasks)
    Xb = dd.binned().numpy()
    fb = forest_ops.build_cpu(Xb, dd.y_enc.astype(np.int32), None, dd.roles_np(), specs, dd.n_classes, False)
    rows = np.arange(0, N, 2, dtype=np.int32)
    sub = np.array([[3, 200, 90, 3], [0, 255, 17, 100]], dtype=np.uint8)    # feature 0's list holds a duplicate bin
    kw = dict(want_rows=True, want_walked=True)
    got = forest_ops.partial_dependence_values(fb, Xb, 2, 9, rows, [0, 1], sub, [4, 3], depth_cap=3, **kw)
    cut = _forest_build(extract_forest(fb, 2, 9, dd, tasks[1], depth_cap=3))
    ref = forest_ops.partial_dependence_values(cut, Xb, 0, 7, rows, [0, 1], sub, [4, 3], **kw)
    whole = forest_ops.partial_dependence_values(fb, Xb, 2, 9, rows, [0, 1], sub, [4, 3], **kw)
    for key in ("rows", "base_rows"):
        np.testing.assert_array_equal(got[key].numpy(), ref[key].numpy())
    np.testing.assert_array_equal(got["average"], ref["average"])
    np.testing.assert_array_equal(got["walked"], ref["walked"])
    assert not np.array_equal(got["rows"].numpy(), whole["rows"].numpy())     # the cap is read
    np.testing.assert_array_equal(got["average"][0, 0], got["average"][0, 3])  # the duplicate bin: copied
    assert np.isnan(got["average"][1, 3]).all()                                # past n_grid
    # the baseline slot is the plain predict_proba of those trees
    _, proba = forest_ops.predict(cut, Xb, np.array([0, 7]), np.array([0, len(rows)]), rows, want_proba=True)
    np.testing.assert_array_equal(ref["base_rows"].numpy(), proba)
    # no_skip: the same values, more walks
    ns = forest_ops.partial_dependence_values(fb, Xb, 2, 9, rows, [0, 1], sub, [4, 3], depth_cap=3, no_skip=True, **kw)
    np.testing.assert_array_equal(ns["rows"].numpy(), got["rows"].numpy())
    assert (ns["walked"] > got["walked"]).all() and got["walked"].sum() > 0


def test_too_close_feature_is_left_out_with_a_warning():
    X, y = _table(0)
    X[:, 2] = 0.0
    X[:40, 2] = np.arange(40)                    # 40 distinct values >= G, both percentiles on the zeros
    dd = DeviceData(X, y, False, "cpu")
    dd.set_splits(np.ones((1, N), np.uint8), ["full"])
    fam = family_of(REG)
    task = FitTask(0, 0, 0, REG, fam.resolve(REG, {"n_estimators": 3, "random_state": 0}, N, D, 1))
    task.partial_dependence = {"features": None, "grid_resolution": G, "percentiles": [0.3, 0.8], "max_rows": None,
                               "random_state": 0}
    out = fam.run(dd, [task], keep_models=True)[0]
    msg = "partial_dependence: feature 2: percentiles are too close to each other"
    assert msg in out.info["warnings"] and out.model["pd_meta"]["warnings"] == [msg]
    np.testing.assert_array_equal(out.model["pd_features"], [0, 1, 3, 4, 5])


def test_binned_only_table_computes_nothing_and_warns():
    from cs230_distributed_machine_learning_amd.models.forest import PD_BINNED

    X, y = _table(3)
    dd = DeviceData(X, y, True, "cpu")
    dd.set_splits(np.ones((1, N), np.uint8), ["full"])
    dd.binned()
    dd.bin_values()                              # cached: the fit below needs no float32 rows
    dd.X = None                                  # as a table resident only in binned form
    fam = family_of(CLS)
    task = FitTask(0, 0, 0, CLS, fam.resolve(CLS, {"n_estimators": 3, "random_state": 0}, N, D, 3))
    task.partial_dependence = {"features": None, "grid_resolution": G, "percentiles": [0.05, 0.95], "max_rows": None,
                               "random_state": 0}
    out = fam.run(dd, [task], keep_models=True)[0]
    assert out.info["warnings"].count(PD_BINNED) == 1 and "float32 rows" in PD_BINNED
    assert out.model is not None and not [k for k in out.model if k.startswith("pd_")]


# ---- opting out, and what is refused ----------------------------------------------------------
def test_job_without_the_option_has_none_of_it(ctl, tmp_path):
    m, _X = _client(ctl, tmp_path, 3)
    out = _train(m, GridSearchCV(RandomForestClassifier(n_estimators=5), {"max_depth": [2]}, cv=2), None)
    assert out["job_status"] == "completed"
    assert all("partial_dependence" not in r for r in out["job_result"]["results"])
    assert "partial_dependence" not in (out.get("best_result") or {})
    est = m.download_best_model(dest=str(tmp_path / "plain.npz"), load=True)
    assert not [k for k in load_model(str(tmp_path / "plain.npz")) if k.startswith("pd_")]
    with pytest.raises(AttributeError, match=r'train_params\["partial_dependence"\]'):
        est.partial_dependence(0)
    assert "partial_dependence" not in job_plan({"model_details": {"model_type": CLS, "hyperparameters": {}}})


def test_keep_models_none_computes_nothing(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), device="cpu", keep_models="none"))
    try:
        m, _X = _client(c, tmp_path, 3)
        out = _train(m, GridSearchCV(RandomForestClassifier(n_estimators=5), {"max_depth": [2]}, cv=2), True)
        assert out["job_status"] == "completed", out
        assert all("partial_dependence" not in r for r in out["job_result"]["results"])
        assert "partial_dependence" not in (out.get("best_result") or {})
    finally:
        c.shutdown()


@pytest.mark.parametrize("option,message", [
    ("yes", "must be true or a dict"),
    ({"grid": 3}, "unknown key(s) ['grid']"),
    ({"features": []}, "features must be None or a list of distinct column positions"),
    ({"features": [1, 1]}, "features must be None or a list of distinct column positions"),
    ({"features": [-1]}, "features must be None or a list of distinct column positions"),
    ({"features": "f0"}, "features must be None or a list of distinct column positions"),
    ({"grid_resolution": 1}, "grid_resolution must be an int >= 2"),
    ({"grid_resolution": 2.5}, "grid_resolution must be an int >= 2"),
    ({"percentiles": [0.5, 0.5]}, "percentiles must be [lo, hi]"),
    ({"percentiles": [0.1, 1.5]}, "percentiles must be [lo, hi]"),
    ({"percentiles": [0.1]}, "percentiles must be [lo, hi]"),
    ({"max_rows": 0}, "max_rows must be None or an int >= 1"),
    ({"random_state": None}, "random_state must be an int"),
    ({"random_state": -1}, "random_state must be an int"),
])
def test_option_errors(option, message):
    from cs230_distributed_machine_learning_amd.engine.service import partial_dependence_options

    with pytest.raises(ParamError) as e:
        partial_dependence_options({"partial_dependence": option}, CLS)
    assert message in str(e.value)


def test_options_resolve():
    from cs230_distributed_machine_learning_amd.engine.service import partial_dependence_options

    assert partial_dependence_options({}, CLS) is None and partial_dependence_options({"partial_dependence": False}, CLS) is None
    assert partial_dependence_options({"partial_dependence": True}, REG) == {
        "features": None, "grid_resolution": 100, "percentiles": [0.05, 0.95], "max_rows": 50_000, "random_state": 0}
    got = partial_dependence_options({"partial_dependence": {"features": (2, 0), "percentiles": (0, 1), "max_rows": None}}, CLS)
    assert got["features"] == [2, 0] and got["percentiles"] == [0.0, 1.0] and got["max_rows"] is None


def test_non_forest_model_is_refused(ctl, tmp_path):
    from sklearn.ensemble import GradientBoostingClassifier

    m, _X = _client(ctl, tmp_path, 3)
    out = _train(m, GridSearchCV(GradientBoostingClassifier(n_estimators=3), {"max_depth": [2]}, cv=2), True)
    assert out.get("status") == "error", out
    assert "RandomForestClassifier and RandomForestRegressor, not GradientBoostingClassifier" in out["message"]
    out = _train(m, GridSearchCV(RandomForestClassifier(n_estimators=3), {"max_depth": [2]}, cv=2), {"grid_resolution": 1})
    assert out.get("status") == "error" and "grid_resolution must be an int >= 2" in out["message"], out


def test_refit_model_is_the_entry_point_of_the_cluster_refit():
    """``service.refit_model`` alone (what the cluster runner's rank 0 calls) attaches the arrays."""
    X, y = _table(0)
    plan = job_plan({"model_details": {"model_type": REG, "hyperparameters": {"n_estimators": 3}},
                     "train_params": {"partial_dependence": {**OPTS, "features": [0]}}})
    model = refit_model(plan, {"n_estimators": 3, "random_state": 0}, DeviceData(X, y, False, "cpu"))
    assert all(k in model for k in PD_KEYS) and model["pd_average"].shape == (1, G)
    plain = refit_model({k: v for k, v in plan.items() if k != "partial_dependence"},
                        {"n_estimators": 3, "random_state": 0}, DeviceData(X, y, False, "cpu"))
    assert not [k for k in plain if k.startswith("pd_")]

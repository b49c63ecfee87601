"""Permutation importance of kept RandomForest* models on their held-out rows
(docs/PERMUTATION_IMPORTANCE.md): the host walk (csrc/runtime/forest_perm_cpu.cpp) against
``sklearn.inspection.permutation_importance`` itself, the depth cap and a mid-pool tree range
against the extracted forest, and the plumbing from ``train_params`` to the result, the
artefacts and ``Predictor.permutation_importance_``.

Shapes: 300 rows and 6 features (2 informative, feature 5 constant: no tree can split on it),
7 trees of unlimited depth; a holdout of 60 rows."""
import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.engine.model_store import Predictor, _forest_build, load_model
from cs230_distributed_machine_learning_amd.engine.service import Controller
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.models.forest import extract_forest
from cs230_distributed_machine_learning_amd.ops import forest_ops

sk = pytest.importorskip("sklearn")
from sklearn.base import BaseEstimator  # noqa: E402
from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor  # noqa: E402
from sklearn.inspection import permutation_importance as sk_permutation_importance  # noqa: E402
from sklearn.model_selection import GridSearchCV, train_test_split  # noqa: E402

CLS, REG = "RandomForestClassifier", "RandomForestRegressor"
N, D = 300, 6
NEW_KEYS = ("permutation_importances", "permutation_importances_mean", "permutation_importances_std",
            "permutation_baseline_score", "permutation_rows", "permutation_meta")


def _table(is_cls):
    rng = np.random.RandomState(5)
    X = rng.normal(size=(N, D)).astype(np.float32)
    X[:, 5] = 1.0
    z = 2.0 * X[:, 0] - X[:, 1] + 0.1 * rng.normal(size=N)
    if is_cls:
        return X, np.searchsorted(np.quantile(z, [1 / 3, 2 / 3]), z).astype(np.int64)   # C = 3
    return X, z.astype(np.float32)


class _Fitted(BaseEstimator):
    """The artefact's Predictor as a fitted sklearn estimator (``fit`` does nothing)."""

    def __init__(self, predictor=None, is_cls=True):
        self.predictor = predictor
        self.is_cls = is_cls

    def fit(self, X, y=None):
        return self

    def predict(self, X):
        p = self.predictor.predict(np.asarray(X, dtype=np.float32))
        return p if self.is_cls else p.astype(np.float64)


def _kept_model(is_cls, scoring):
    X, y = _table(is_cls)
    name = CLS if is_cls else REG
    opts = {"n_repeats": 3, "random_state": 7, "scoring": scoring, "candidates": "all"}
    spec = JobSpec(name, [{"n_estimators": 7, "random_state": 3}], cv=0, holdout=True, keep_models="all",
                   permutation=opts)
    r = run_candidates(DeviceData(X, y, is_cls, "cpu"), spec, [0])[0]
    assert r.ok, r.error
    return X, y, r


def test_permutation_indices_is_the_numpy_stream():
    for K in (1, 5):
        got = forest_ops.permutation_indices(37, K, 11)
        assert got.dtype == np.int32 and got.shape == (K, 37)
        r = np.random.RandomState(np.random.RandomState(11).randint(np.iinfo(np.int32).max + 1))
        col, idx = np.arange(37), np.arange(37)   # sklearn shuffles one index array in place, repeat after
        for k in range(K):                         # repeat, and permutes the already permuted column again
            r.shuffle(idx)
            col = col[idx]
            np.testing.assert_array_equal(got[k], col)
            assert sorted(got[k]) == list(range(37))


@pytest.mark.parametrize("is_cls,scoring", [(True, "accuracy"), (False, "r2"), (False, "neg_mean_squared_error"),
                                            (False, "neg_root_mean_squared_error")])
def test_importances_are_sklearns(is_cls, scoring):
    X, y, r = _kept_model(is_cls, scoring)
    m = r.model
    rows = m["permutation_rows"]
    np.testing.assert_array_equal(rows, np.sort(train_test_split(np.arange(N), test_size=0.2, random_state=42)[1]))
    y_rows = y[rows] if is_cls else y[rows].astype(np.float64)        # the float32 target, widened
    ref = sk_permutation_importance(_Fitted(Predictor(m), is_cls), X[rows], y_rows, scoring=scoring, n_repeats=3,
                                    random_state=7)
    imp = m["permutation_importances"]
    assert imp.shape == (D, 3) and imp.dtype == np.float64
    print(scoring, "max |ours - sklearn| =", np.abs(imp - ref.importances).max())
    if is_cls:
        assert np.abs(imp - ref.importances).max() <= 1e-15
    else:
        np.testing.assert_allclose(imp, ref.importances, rtol=1e-12, atol=0)
    assert not np.any(imp[5]) and not np.any(ref.importances[5])       # the constant feature: exactly zero
    assert np.abs(imp[:2]).min() > 0.05                                  # the informative ones are not
    np.testing.assert_array_equal(m["permutation_importances_mean"], imp.mean(1))
    np.testing.assert_array_equal(m["permutation_importances_std"], imp.std(1))
    entry = r.result["permutation_importance"]
    assert entry["scoring"] == scoring and entry["n_repeats"] == 3 and entry["random_state"] == 7
    assert entry["importances_mean"] == list(imp.mean(1))
    main = {"accuracy": "accuracy", "r2": "r2_score"}.get(scoring)
    if main:
        assert entry["baseline_score"] == r.result[main]
    elif scoring == "neg_mean_squared_error":
        assert entry["baseline_score"] == -r.result["mean_squared_error"]


@pytest.mark.parametrize("is_cls", [True, False])
def test_depth_cap_and_mid_pool_range_equal_the_extracted_forest(is_cls):
    """Trees [2, 9) of a pool read down to depth 3 == the same trees extracted and truncated."""
    X, y = _table(is_cls)
    name = CLS if is_cls else REG
    dd = DeviceData(X, y, is_cls, "cpu")
    roles = np.ones((1, N), np.uint8)
    roles[0, ::4] = 2
    dd.set_splits(roles, ["holdout"])
    fam = family_of(name)
    tasks = [FitTask(i, i, 0, name, fam.resolve(name, {"n_estimators": T, "random_state": 5 + i}, 225, D,
                                                 dd.n_classes)) for i, T in enumerate((2, 7))]
    specs = fam._specs(tasks)
    Xb = dd.binned().numpy()
    ycls = None if not is_cls else dd.y_enc.astype(np.int32)
    yreg = None if is_cls else dd.y_reg.numpy()
    fb = forest_ops.build_cpu(Xb, ycls, yreg, dd.roles_np(), specs, dd.n_classes if is_cls else 1, not is_cls)
    rows = dd.test_rows[0].numpy()
    perm = forest_ops.permutation_indices(len(rows), 2, 1)
    kw = dict(ycls=ycls, yreg=yreg, want_pred=True)
    got = forest_ops.permutation_scores(fb, Xb, 2, 9, rows, perm, depth_cap=3, **kw)
    cut = _forest_build(extract_forest(fb, 2, 9, dd, tasks[1], depth_cap=3))
    ref = forest_ops.permutation_scores(cut, Xb, 0, 7, rows, perm, **kw)
    whole = forest_ops.permutation_scores(fb, Xb, 2, 9, rows, perm, **kw)
    for key in ("pred", "base_pred", "sums", "base"):
        np.testing.assert_array_equal(got[key].numpy(), ref[key].numpy())
    assert not np.array_equal(got["pred"].numpy(), whole["pred"].numpy())   # the cap is read
    # and the baseline slot is the plain predict of those trees
    plain = forest_ops.predict(cut, Xb, np.array([0, 7]), np.array([0, len(rows)]), rows.astype(np.int32))
    np.testing.assert_array_equal(ref["base_pred"].numpy(), plain)


# ---- end to end through the client ---------------------------------------------------------
@pytest.fixture
def ctl(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), journal=str(tmp_path / "journal.jsonl"), device="cpu",
                          sse_interval_s=0.05))
    yield c
    c.shutdown()


def _client(ctl, tmp_path, is_cls):
    import pandas as pd
    from distributed_ml import MLTaskManager

    X, y = _table(is_cls)
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D)])
    df["target"] = y
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    m = MLTaskManager(controller=ctl)
    assert "error" not in m.download_data(path, "toy", "local")
    return m, y


def _train(m, est, option, **extra):
    tp = {"target_column": "target", **extra}
    if option is not None:
        tp["permutation_importance"] = option
    return m.train(est, "toy", tp, wait_for_completion=True, polling_interval=0.02)


@pytest.mark.parametrize("is_cls", [True, False])
def test_job_best_candidate(ctl, tmp_path, is_cls):
    m, y = _client(ctl, tmp_path, is_cls)
    base = RandomForestClassifier(n_estimators=7) if is_cls else RandomForestRegressor(n_estimators=7)
    out = _train(m, GridSearchCV(base, {"max_depth": [2, None]}, cv=3), {"n_repeats": 3, "random_state": None})
    assert out["job_status"] == "completed", out
    best = out["best_result"]
    entry = best["permutation_importance"]
    # one more fit of the winner with its own seed: the same trees, so the same holdout score
    assert entry["baseline_score"] == best["accuracy" if is_cls else "r2_score"]
    assert entry["scoring"] == ("accuracy" if is_cls else "r2") and entry["n_repeats"] == 3
    assert isinstance(entry["random_state"], int)                      # the drawn seed is reported
    assert len(entry["importances_mean"]) == D and entry["importances_mean"][5] == 0.0
    assert max(entry["importances_mean"][:2]) > 0.05
    others = [r for r in out["job_result"]["results"] if r["parameters"] != best["parameters"]]
    assert others and all("permutation_importance" not in r for r in others)
    est = m.download_best_model(dest=str(tmp_path / "best.npz"), load=True)   # the refit artefact
    pi = est.permutation_importance_
    assert list(pi.importances_mean) == entry["importances_mean"]
    assert list(pi.importances_std) == entry["importances_std"]
    assert pi.baseline_score == entry["baseline_score"] and pi.importances is None
    assert (pi.scoring, pi.n_repeats, pi.random_state) == (entry["scoring"], 3, entry["random_state"])
    np.testing.assert_array_equal(pi.rows, np.sort(train_test_split(np.arange(N), test_size=0.2, random_state=42)[1]))
    raw = load_model(str(tmp_path / "best.npz"))
    assert "permutation_importances" not in raw and all(k in raw for k in NEW_KEYS[1:5])


def test_job_all_candidates_and_holdout_artefacts(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), device="cpu", keep_models="all"))
    try:
        m, y = _client(c, tmp_path, True)
        out = _train(m, GridSearchCV(RandomForestClassifier(n_estimators=7, random_state=1), {"max_depth": [2, None]}, cv=3),
                     {"n_repeats": 2, "candidates": "all", "random_state": 4})
        assert out["job_status"] == "completed", out
        res = out["job_result"]["results"]
        assert len(res) == 2
        for r in res:
            e = r["permutation_importance"]
            assert e["baseline_score"] == r["accuracy"] and e["random_state"] == 4 and e["n_repeats"] == 2
        assert res[0]["permutation_importance"]["importances_mean"] != res[1]["permutation_importance"]["importances_mean"]
        best = out["best_result"]
        loser = [r for r in res if r["parameters"] != best["parameters"]][0]
        hold = Predictor(load_model(loser["model_path"]))                # a holdout fit's own artefact
        pi = hold.permutation_importance_
        assert pi.importances.shape == (D, 2)
        assert list(pi.importances.mean(1)) == loser["permutation_importance"]["importances_mean"]
        refit = Predictor(load_model(best["model_path"])).permutation_importance_
        assert list(refit.importances_mean) == best["permutation_importance"]["importances_mean"]
    finally:
        c.shutdown()


@pytest.mark.parametrize("option,extra,est,message", [
    ({"n_repeats": 0}, {}, None, "n_repeats must be an int >= 1"),
    ({"n_repeats": 2.5}, {}, None, "n_repeats must be an int >= 1"),
    ({"scoring": "f1_macro"}, {}, None, "supported: ['accuracy']"),
    ({"candidates": "some"}, {}, None, "candidates must be 'best' or 'all'"),
    ({"repeats": 3}, {}, None, "unknown key(s) ['repeats']"),
    (True, {"holdout": False}, None, "needs holdout=True"),
    (True, {}, "other", "RandomForestClassifier and RandomForestRegressor, not GradientBoostingClassifier"),
])
def test_validation_errors(ctl, tmp_path, option, extra, est, message):
    from sklearn.ensemble import GradientBoostingClassifier

    m, _y = _client(ctl, tmp_path, True)
    base = GradientBoostingClassifier(n_estimators=3) if est == "other" else RandomForestClassifier(n_estimators=3)
    out = _train(m, GridSearchCV(base, {"max_depth": [2]}, cv=2), option, **extra)
    assert out.get("status") == "error" and message in out["message"], out


def test_regressor_scoring_is_validated(ctl, tmp_path):
    m, _y = _client(ctl, tmp_path, False)
    out = _train(m, GridSearchCV(RandomForestRegressor(n_estimators=3), {"max_depth": [2]}, cv=2), {"scoring": "accuracy"})
    assert out.get("status") == "error" and "'r2', 'neg_mean_squared_error', 'neg_root_mean_squared_error'" in out["message"]


def test_job_without_the_option_has_none_of_it(ctl, tmp_path):
    m, _y = _client(ctl, tmp_path, True)
    out = _train(m, GridSearchCV(RandomForestClassifier(n_estimators=5), {"max_depth": [2]}, cv=2), None)
    assert out["job_status"] == "completed"
    assert all("permutation_importance" not in r for r in out["job_result"]["results"])
    path = m.download_best_model(dest=str(tmp_path / "plain.npz"))
    raw = load_model(path)
    assert not [k for k in raw if k.startswith("permutation")]
    with pytest.raises(AttributeError, match=r'train_params\["permutation_importance"\]'):
        Predictor(raw).permutation_importance_

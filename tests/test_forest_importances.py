"""feature_importances_ of kept RandomForest* models against sklearn (mean decrease in impurity).

With no bootstrap, every feature and exactly binned data each tree is sklearn's tree, so the
importances must agree to rounding -- wherever sklearn agrees with itself: deeper trees on these
data have equal-gain ties that sklearn breaks by its random feature order (its own importances
then differ by 0.01-0.03 between two random_state values).  Depth 4 is tie-free for every case
below, which each test asserts first."""
import os

import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.model_store import Predictor, load_predictor, save_model
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.ops import forest_ops

sk = pytest.importorskip("sklearn")
from sklearn.datasets import make_classification, make_regression  # noqa: E402
from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor  # noqa: E402

COMMON = {"bootstrap": False, "max_features": None, "max_depth": 4}
_DATA = {}


def _data(is_cls):
    if is_cls not in _DATA:
        if is_cls:
            X, y = make_classification(600, 6, n_informative=5, n_redundant=0, n_classes=3, random_state=11)
            X = np.round(X, 1)
        else:
            X, y = make_regression(500, 5, noise=5, random_state=12)
            X, y = np.round(X, 1), np.round(y, 2)
        dd = DeviceData(X, y, is_cls, "cpu")
        dd.set_splits(np.ones((1, len(y)), np.uint8), ["full"])
        _DATA[is_cls] = (X, y, dd)
    return _DATA[is_cls]


def _fit(is_cls, params, dd=None):
    name = "RandomForestClassifier" if is_cls else "RandomForestRegressor"
    X, y, dd0 = _data(is_cls)
    dd = dd or dd0
    fam = family_of(name)
    rp = fam.resolve(name, params, dd.train_counts[0], dd.d, dd.n_classes)
    return fam.run(dd, [FitTask(0, 0, 0, name, rp)], keep_models=True)[0].model


def _sklearn(is_cls, params):
    X, y, _ = _data(is_cls)
    est = RandomForestClassifier if is_cls else RandomForestRegressor
    a, b = (est(random_state=s, **params).fit(X, y).feature_importances_ for s in (0, 1))
    # precondition: the case is tie-free, sklearn agrees with itself
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    return a


@pytest.mark.parametrize("criterion", ["gini", "entropy"])
@pytest.mark.parametrize("extra", [{}, {"class_weight": "balanced"}, {"ccp_alpha": 0.01}, {"max_leaf_nodes": 7},
                                   {"min_samples_leaf": 20}], ids=lambda e: next(iter(e), "plain"))
def test_classifier_importances_match_sklearn(criterion, extra):
    params = dict(COMMON, n_estimators=3, criterion=criterion, **extra)
    ref = _sklearn(True, params)
    m = _fit(True, params)
    fi = m["feature_importances"]
    assert fi.dtype == np.float64 and fi.shape == (6,)
    np.testing.assert_allclose(fi, ref, rtol=0, atol=1e-12)
    assert (fi >= 0).all() and abs(fi.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("criterion", ["squared_error", "friedman_mse"])
def test_regressor_importances_match_sklearn(criterion):
    params = dict(COMMON, n_estimators=3, criterion=criterion)
    ref = _sklearn(False, params)
    fi = _fit(False, params)["feature_importances"]
    np.testing.assert_allclose(fi, ref, rtol=0, atol=1e-8)
    assert (fi >= 0).all() and abs(fi.sum() - 1.0) < 1e-12


def test_all_single_leaf_forest_gives_zeros():
    # min_samples_split above the row count: every tree is its root
    m = _fit(True, dict(COMMON, n_estimators=4, min_samples_split=10000))
    assert (m["nodes"][:, 0] < 0).all() and len(m["nodes"]) == 4
    np.testing.assert_array_equal(m["feature_importances"], np.zeros(6))
    np.testing.assert_array_equal(Predictor(m).feature_importances_, np.zeros(6))


def test_bootstrap_forest_importances_are_a_distribution():
    m = _fit(True, {"n_estimators": 20, "random_state": 5})
    fi = Predictor(m).feature_importances_
    assert (fi >= 0).all() and abs(fi.sum() - 1.0) < 1e-12
    # the uninformative-feature-free table: every feature is used somewhere in 20 full trees
    assert (fi > 0).all()


@pytest.mark.parametrize("criterion", ["poisson", "absolute_error"])
def test_criteria_without_pool_impurity_raise(criterion):
    X, y, _ = _data(False)
    dd = DeviceData(X, np.abs(y), False, "cpu")
    dd.set_splits(np.ones((1, len(y)), np.uint8), ["full"])
    m = _fit(False, {"n_estimators": 2, "max_depth": 3, "criterion": criterion}, dd)
    assert "feature_importances" not in m
    with pytest.raises(AttributeError, match=criterion):
        Predictor(m).feature_importances_
    # ... and the prediction path of such an artefact is untouched
    assert Predictor(m).predict(X[:5]).shape == (5,)


def test_round_trip_and_lazy_importances(tmp_path):
    m = _fit(True, dict(COMMON, n_estimators=3, criterion="entropy"))
    path = save_model(m, os.path.join(tmp_path, "rf.npz"))
    est = load_predictor(path)
    np.testing.assert_array_equal(est.feature_importances_, m["feature_importances"])
    # an artefact saved before the vector existed computes it from nodes / vals / params
    old = {k: v for k, v in m.items() if k != "feature_importances"}
    np.testing.assert_array_equal(Predictor(old).feature_importances_, m["feature_importances"])
    path = save_model(old, os.path.join(tmp_path, "rf_old.npz"))
    np.testing.assert_array_equal(load_predictor(path).feature_importances_, m["feature_importances"])
    with pytest.raises(AttributeError):
        est.oob_score_
    with pytest.raises(AttributeError):
        load_predictor(path).oob_decision_function_


def test_non_forest_artefact_has_no_importances():
    with pytest.raises(AttributeError):
        Predictor({"kind": "linear_regression", "coef": np.zeros(3), "intercept": 0.0}).feature_importances_


def test_depth_capped_prefix_equals_the_fit_grown_alone(monkeypatch):
    """A max_depth prefix follower is extracted from its leader's deeper trees with a depth cap
    (nodes at the cap become leaves): its importances are those of the fit grown alone."""
    from cs230_distributed_machine_learning_amd.models.forest import _refine, extract_forest

    monkeypatch.setenv("DML_PREFIX_SHARE", "0")
    X, y, dd = _data(True)
    fam = family_of("RandomForestClassifier")
    deep = dict(n_estimators=5, max_depth=8, random_state=3)
    shallow = dict(n_estimators=3, max_depth=3, random_state=3)
    alone = _fit(True, shallow)
    # the leader's pool, cut the way _run_batch cuts it for the follower
    rp = fam.resolve("RandomForestClassifier", deep, dd.train_counts[0], dd.d, dd.n_classes)
    task = FitTask(0, 0, 0, "RandomForestClassifier", rp)
    specs = fam._specs([task])
    fb = forest_ops.build_cpu(dd.binned().numpy(), dd.y_enc, None, dd.roles_np(), specs, dd.n_classes, False)
    _refine(dd, fb, dd.binned(), specs, dd.roles)
    rp_f = fam.resolve("RandomForestClassifier", shallow, dd.train_counts[0], dd.d, dd.n_classes)
    capped = extract_forest(fb, 0, 3, dd, FitTask(1, 0, 0, "RandomForestClassifier", rp_f), depth_cap=3)
    np.testing.assert_array_equal(capped["nodes"], alone["nodes"])
    np.testing.assert_array_equal(capped["feature_importances"], alone["feature_importances"])
    full = extract_forest(fb, 0, 5, dd, task)
    assert np.abs(full["feature_importances"] - alone["feature_importances"]).max() > 1e-6

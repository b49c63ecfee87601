"""LinearDiscriminantAnalysis on the CPU data path (models/discriminant.py, docs/LDA.md) against
sklearn: a grid over solver x shrinkage x priors, every kept fit against sklearn's estimator on the
same rows, and sklearn's error and warning texts.

Measured deviations of a kept model from sklearn float64, largest over the three tables and all
fits, each relative to the largest magnitude of sklearn's array (printed; run with ``-s``):
``decision_function`` 1.41e-14 (off-origin table, svd), ``coef_`` 8.06e-15, ``intercept_`` 4.96e-15,
``covariance_`` 4.85e-16.  The two sides order their d-term sums differently (moments and ``eigh``
here, centred rows and ``lstsq`` / SVD there); the bounds are 10 x the measured values.
"""
import warnings

import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine import model_store
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, build_tasks, prepare_splits, run_candidates
from cs230_distributed_machine_learning_amd.models import discriminant
from cs230_distributed_machine_learning_amd.models.base import family_of

sk = pytest.importorskip("sklearn")
from sklearn.discriminant_analysis import LinearDiscriminantAnalysis  # noqa: E402
from sklearn.model_selection import GridSearchCV  # noqa: E402

LDA = "LinearDiscriminantAnalysis"
TABLES = {"binary": (130, 9, 2, 0.0), "four_class": (200, 17, 4, 0.0), "off_origin": (150, 7, 3, 50.0)}
DEC_TOL, COEF_TOL, ICPT_TOL, COV_TOL = 1.41e-13, 8.06e-14, 4.96e-14, 4.85e-15   # 10 x the measured worst


def table(n, d, C, off=0.0):
    rng = np.random.default_rng(0)
    y = rng.integers(0, C, n)
    X = (rng.normal(size=(n, d)) * np.linspace(0.5, 3, d) + 0.7 * y[:, None] + off).astype(np.float32)
    return X, y


def grid(C):
    """svd, lsqr and eigen at every shrinkage, and two candidates with given priors."""
    pri = (np.arange(1, C + 1) / np.arange(1, C + 1).sum()).tolist()
    return ([{"solver": "svd"}] + [{"solver": s, "shrinkage": a} for s in ("lsqr", "eigen") for a in (None, 0.3, 1.0, "auto")]
            + [{"solver": "lsqr", "shrinkage": "auto", "priors": pri}, {"solver": "svd", "priors": pri}])


@pytest.mark.parametrize("name", list(TABLES))
def test_grid_and_kept_models_match_sklearn(tmp_path, name):
    n, d, C, off = TABLES[name]
    X, y = table(n, d, C, off)
    X64, g = X.astype(np.float64), grid(C)
    ref = GridSearchCV(LinearDiscriminantAnalysis(), [{k: [v] for k, v in p.items()} for p in g], cv=3).fit(X64, y)
    dd = DeviceData(X, y, True, "cpu")
    res = run_candidates(dd, JobSpec(LDA, g, cv=3, holdout=False), range(len(g)))
    for i, r in enumerate(res):
        assert r.ok, r.error
        assert r.result["cv_scores"] == [ref.cv_results_[f"split{k}_test_score"][i] for k in range(3)], g[i]
    assert int(np.argmax([r.result["mean_cv_score"] for r in res])) == ref.best_index_
    spec = JobSpec(LDA, g, cv=3, keep_models="all", holdout=False)
    prepare_splits(dd, spec)
    tasks, errors = build_tasks(dd, spec, range(len(g)))
    assert not errors, errors
    worst = np.zeros(4)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for t, o in zip(tasks, family_of(LDA).run(dd, tasks, keep_models=True)):
        tr, te = dd.train_rows[t.split].long().numpy(), dd.test_rows[t.split].long().numpy()
        skm = LinearDiscriminantAnalysis(**{k: t.params[k] for k in ("solver", "shrinkage", "priors")}).fit(X64[tr], y[tr])
        est = model_store.Predictor(model_store.load_model(model_store.save_model(o.model, str(tmp_path / "m.npz"))))
        dec, want = est.decision_function(X[te]), skm.decision_function(X64[te])
        assert dec.shape == want.shape and est.coef_.shape == skm.coef_.shape and est.intercept_.shape == skm.intercept_.shape
        cov = rel(est.covariance_, skm.covariance_) if t.params["solver"] != "svd" else 0.0
        worst = np.maximum(worst, [rel(dec, want), rel(est.coef_, skm.coef_), rel(est.intercept_, skm.intercept_), cov])
        assert (est.predict(X[te]) == skm.predict(X64[te])).all() and (o.pred.numpy() == np.searchsorted(
            skm.classes_, skm.predict(X64[te]))).all()
        # softmax moves by at most twice the largest change of its arguments
        np.testing.assert_allclose(est.predict_proba(X[te]), skm.predict_proba(X64[te]), rtol=0,
                                   atol=2 * DEC_TOL * np.abs(want).max())
        # a mean of at most n terms below max|x|, summed in two orders
        np.testing.assert_allclose(est.means_, skm.means_, rtol=0, atol=n * np.finfo(np.float64).eps * np.abs(X64).max())
        np.testing.assert_allclose(est.priors_, skm.priors_, rtol=1e-15)
    print(f"kept models vs sklearn on {name}: decision, coef_, intercept_, covariance_ =", worst)
    assert (worst <= [DEC_TOL, COEF_TOL, ICPT_TOL, COV_TOL]).all(), worst


@pytest.mark.parametrize("params,where,text", [
    ({"solver": "svd", "shrinkage": 0.3}, "fit", discriminant.SVD_SHRINKAGE),
    ({"solver": "svd", "shrinkage": "auto"}, "fit", discriminant.SVD_SHRINKAGE),
    ({"n_components": 3}, "param", discriminant.BAD_COMPONENTS),
    ({"solver": "lsqr", "covariance_estimator": "OAS"}, "param", "covariance_estimator"),
    ({"solver": "qr"}, "param", "solver"),
    ({"solver": "lsqr", "shrinkage": 1.5}, "param", "shrinkage"),
    ({"priors": [-0.5, 1.0, 0.5]}, "param", "priors must be non-negative"),
    ({"priors": [2.0, 1.0, 1.0]}, "warning", discriminant.PRIORS_RENORM),
    ({"bogus": 1}, "warning", "ignored unknown parameters ['bogus']"),
])
def test_errors_and_warnings_follow_sklearn(params, where, text):
    X, y = table(96, 5, 3)
    r = run_candidates(DeviceData(X, y, True, "cpu"), JobSpec(LDA, [params], cv=3, holdout=False), [0])[0]
    if where == "warning":
        assert r.ok and text in r.result["warnings"]
        skp = {k: v for k, v in params.items() if k != "bogus"}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # sklearn's own renormalising warning
            skm = GridSearchCV(LinearDiscriminantAnalysis(**skp), {}, cv=3).fit(X.astype(np.float64), y)
        assert r.result["cv_scores"] == [skm.cv_results_[f"split{k}_test_score"][0] for k in range(3)]
    else:
        assert not r.ok and text in r.error and ("ParamError" in r.error) == (where == "param")


def test_singular_covariance_eigen_fails_lsqr_is_minimum_norm():
    """A constant column: the covariance has an exactly zero row on both sides."""
    X, y = table(96, 5, 3)
    X[:, 4] = 2.0
    X64 = X.astype(np.float64)
    res = run_candidates(DeviceData(X, y, True, "cpu"), JobSpec(LDA, [{"solver": "eigen"}, {"solver": "lsqr"}], cv=3,
                                                                 holdout=False), [0, 1])
    with pytest.raises(np.linalg.LinAlgError) as e:
        LinearDiscriminantAnalysis(solver="eigen").fit(X64, y)
    assert not res[0].ok and str(e.value) in res[0].error
    ref = GridSearchCV(LinearDiscriminantAnalysis(solver="lsqr"), {}, cv=3).fit(X64, y)
    assert res[1].ok and res[1].result["cv_scores"] == [ref.cv_results_[f"split{k}_test_score"][0] for k in range(3)]

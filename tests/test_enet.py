"""Ridge, Lasso and ElasticNet on the CPU data path (models/linear.py PenalizedLinearFamily,
docs/ELASTIC_NET.md): the host twin of the solver kernel against sklearn's own solver, sklearn's
duality-gap contract recomputed from the raw rows, jobs through the client against sklearn's
GridSearchCV, and the edge cases.

Recorded deviations (this file prints them; run with ``-s``):

* twin vs ``sklearn.linear_model._cd_fast.enet_coordinate_descent_gram`` over the 432 cases of
  enet_cases.py: ``n_iter`` equal on every case with the seeds as first chosen (no seed was
  replaced); ``w`` equal bit for bit (worst max|dw| / max|w| = 0); worst |dgap| / ynorm2 =
  8.5e-16.  The bound below is 100 x that worst, 8.5e-14, for both quantities.  The gap is
  compared relative to ynorm2 because it is a sum of terms of that size which cancel, and
  because the stopping test compares it with tol * ynorm2.
* Ridge coefficients vs ``Ridge(solver="cholesky")`` on the 600 x 12 table: worst
  max|dcoef| / max|coef| = 1.9e-15 over alphas [0, 1e-3, 1, 1e3] x fit_intercept.
"""
import json
import warnings

import numpy as np
import pytest
import torch

import enet_cases as ec
from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, build_tasks, prepare_splits, run_candidates
from cs230_distributed_machine_learning_amd.engine.service import Controller, refit_model
from cs230_distributed_machine_learning_amd.models import linear
from cs230_distributed_machine_learning_amd.models.base import family_of, supported_models
from cs230_distributed_machine_learning_amd.ops import enet_ops

sk = pytest.importorskip("sklearn")
from sklearn.linear_model import ElasticNet, Lasso, Ridge  # noqa: E402
from sklearn.model_selection import GridSearchCV  # noqa: E402

TWIN_BOUND = 8.5e-14   # 100 x the measured worst deviation (module docstring); never above 1e-9
KEYS = ("Q", "q", "ynorm2", "gram_id", "l1", "l2", "positive", "max_iter", "tol")


def _twin(inp):
    return enet_ops.enet_cd(*[torch.from_numpy(np.array(inp[k])) for k in KEYS])


# ---- the twin against sklearn's solver ------------------------------------------------------------
def test_twin_matches_sklearn_gram_solver():
    from sklearn.linear_model._cd_fast import enet_coordinate_descent_gram

    assert TWIN_BOUND <= 1e-9
    worst_w = worst_gap = 0.0
    mismatched = []
    for d in ec.DS:
        inp, ps = ec.solver_inputs(d)
        w, gap, tol_eff, n_iter = (t.numpy() for t in _twin(inp))
        Q, q, yc = (np.array(a) for a in ec.gram(d))
        yn = float(inp["ynorm2"][0])
        for i, p in enumerate(ps):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")   # ConvergenceWarning / no-L1 warning of the cases that ask for them
                ws, gs, ts, ns = enet_coordinate_descent_gram(
                    np.zeros(d), p["l1"], p["l2"], Q, q, yc, p["max_iter"], p["tol"], np.random.RandomState(0), False,
                    p["positive"])
            if ns != n_iter[i]:
                mismatched.append((d, i, ns, int(n_iter[i])))
                continue
            assert ts == tol_eff[i]
            scale = np.abs(ws).max()
            dw = np.abs(ws - w[i]).max() / scale if scale > 0 else np.abs(w[i]).max()
            worst_w = max(worst_w, float(dw))
            worst_gap = max(worst_gap, abs(gs - gap[i]) / yn)
    print(f"twin vs sklearn: worst max|dw|/max|w| = {worst_w:.3e}, worst |dgap|/ynorm2 = {worst_gap:.3e}, "
          f"n_iter mismatches = {mismatched}")
    assert not mismatched, mismatched
    assert worst_w <= TWIN_BOUND and worst_gap <= TWIN_BOUND


def test_twin_entry_edge_cases():
    inp, _ps = ec.solver_inputs(3)
    none = dict(inp, **{k: inp[k][:0] for k in KEYS[3:]})
    w, gap, tol_eff, n_iter = _twin(none)                         # F = 0
    assert w.shape == (0, 3) and n_iter.numel() == 0
    with pytest.raises(ValueError):
        _twin(dict(inp, gram_id=np.ones_like(inp["gram_id"])))    # a Gram that is not there
    with pytest.raises(ValueError):
        _twin(dict(inp, tol=inp["tol"][:-1]))


# ---- the family ------------------------------------------------------------------------------------
def _family_fits(dd, model, params, cv=3, holdout=False):
    """(tasks, outputs with models) of every (candidate, split) through the family."""
    spec = JobSpec(model, params, cv=cv, holdout=holdout, keep_models="all")
    prepare_splits(dd, spec)
    tasks, errors = build_tasks(dd, spec, range(len(params)))
    assert not errors, errors
    outs = family_of(model).run(dd, tasks, keep_models=True)
    return tasks, outs


def _raw_gap(X, y, coef, intercept, l1, l2, positive, dual_is_zero=False):
    """sklearn's duality gap of (coef, intercept) from the raw training rows, numpy float64
    (``dual_is_zero``: take the ``const = 1`` branch whatever the round-off of the dual norm)."""
    Xc = X - X.mean(0)
    yc = y - y.mean()
    R = y - X @ coef - intercept
    XtA = Xc.T @ R - l2 * coef
    dual = XtA.max() if positive else np.abs(XtA).max()
    Rn = R @ R
    if dual > l1 and not dual_is_zero:
        c = l1 / dual
        gap = 0.5 * (Rn + Rn * c * c)
    else:
        c, gap = 1.0, Rn
    return gap + l1 * np.abs(coef).sum() - c * (R @ yc) + 0.5 * l2 * (1 + c * c) * (coef @ coef), yc @ yc


@pytest.mark.parametrize("d", ec.DS)
def test_converged_fits_meet_sklearns_gap_contract_on_raw_rows(d):
    """Every converged fit of the full case grid, the gap recomputed from the raw rows.

    With an L1 term the recomputation is sklearn's formula as it stands.  Without one
    (``l1 = 0``) the formula has two branches that differ by about ynorm2 / 2: ``dual_norm > 0``
    gives ``const = 0`` and a gap of at least ``R / 2``, so such a fit can only have converged
    through the other branch (``const = 1``), which the solver takes when ``X^T R - l2 w`` rounded
    to exactly 0 in its arithmetic.  Recomputed from the rows in another summation order that
    vector is round-off, not 0.  For those fits the test therefore asserts the premise -- the
    dual norm is 0 to round-off, at most ``1e-9 max|X^T y|`` -- and the bound on the
    ``const = 1`` gap, the branch the solver evaluated."""
    X, y = ec.table(d)
    dd = DeviceData(X, y, False, "cpu")
    grid = [{"alpha": a, "l1_ratio": r, "positive": p, "max_iter": mi, "tol": tol}
            for a in ec.ALPHAS for r in ec.L1_RATIOS for p in ec.POSITIVE for mi, tol in ec.ITER_TOL]
    tasks, outs = _family_fits(dd, "ElasticNet", grid)
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    checked = checked_no_l1 = 0
    for t, o in zip(tasks, outs):
        if any("did not converge" in w for w in o.info["warnings"]):
            continue
        tr = dd.train_rows[t.split].long().numpy()
        n = len(tr)
        rp = t.params
        l1, l2 = rp["alpha"] * rp["l1_ratio"] * n, rp["alpha"] * (1 - rp["l1_ratio"]) * n
        coef, icpt = o.model["coef"], o.model["intercept"]
        if l1 == 0.0:
            Xc = X64[tr] - X64[tr].mean(0)
            yc = y64[tr] - y64[tr].mean()
            XtA = Xc.T @ (y64[tr] - X64[tr] @ coef - icpt) - l2 * coef
            dual = XtA.max() if rp["positive"] else np.abs(XtA).max()
            assert dual <= 1e-9 * np.abs(Xc.T @ yc).max(), (rp, t.split, dual)
            gap, yn = _raw_gap(X64[tr], y64[tr], coef, icpt, l1, l2, rp["positive"], dual_is_zero=True)
            checked_no_l1 += 1
        else:
            gap, yn = _raw_gap(X64[tr], y64[tr], coef, icpt, l1, l2, rp["positive"])
        assert gap < rp["tol"] * yn * (1 + 1e-9), (rp, t.split, gap, rp["tol"] * yn)
        if d > 1:
            assert coef[min(2, d - 1)] == 0.0      # the constant column
        assert o.model["dual_gap"] * n < rp["tol"] * yn * (1 + 1e-9)
        assert o.info["solver"] == "twin"
        checked += 1
    print(f"d = {d}: {checked} converged fits checked, {checked_no_l1} of them without an L1 term")
    assert checked >= len(tasks) // 3, (checked, len(tasks))


# ---- jobs through the client -------------------------------------------------------------------------
N_JOB, D_JOB = 600, 12


def _job_table():
    rng = np.random.RandomState(11)
    X = rng.normal(size=(N_JOB, D_JOB)).astype(np.float32)
    X[:, 3] += 0.6 * X[:, 0]
    coef = np.array([1.5, 0, 0, -0.8, 0, 0.4, 0, 0, 0, 0, 0.05, 0])
    y = (X.astype(np.float64) @ coef + 0.7 + 0.3 * rng.normal(size=N_JOB)).astype(np.float32)
    return X, y


@pytest.fixture
def ctl(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), journal=str(tmp_path / "journal.jsonl"), device="cpu",
                          sse_interval_s=0.05))
    yield c
    c.shutdown()


def _client(ctl, tmp_path):
    import pandas as pd
    from distributed_ml import MLTaskManager

    X, y = _job_table()
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D_JOB)])
    df["target"] = y
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    m = MLTaskManager(controller=ctl)
    assert "error" not in m.download_data(path, "toy", "local")
    return m


def _train(m, est, **extra):
    out = m.train(est, "toy", {"target_column": "target", **extra}, wait_for_completion=True, polling_interval=0.02)
    assert out["job_status"] == "completed", out
    return out


def _against_sklearn(m, tmp_path, search, keys):
    X, y = _job_table()
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    out = _train(m, search)
    ref = search.fit(X64, y64)
    ours = {json.dumps({k: r["parameters"][k] for k in keys}, sort_keys=True): r for r in out["job_result"]["results"]}
    for params, mean in zip(ref.cv_results_["params"], ref.cv_results_["mean_test_score"]):
        r = ours[json.dumps({k: params[k] for k in keys}, sort_keys=True)]
        assert abs(r["mean_cv_score"] - mean) <= 1e-6, (params, r["mean_cv_score"], mean)
    best = out["job_result"]["best_result"]["parameters"]
    assert {k: best[k] for k in keys} == {k: ref.best_params_[k] for k in keys}
    est = m.download_best_model(dest=str(tmp_path / "best.npz"), load=True)
    assert np.abs(est.predict(X) - ref.best_estimator_.predict(X64)).max() <= 1e-6
    return out, ref, est


def test_lasso_and_elasticnet_jobs_match_sklearn_gridsearch(ctl, tmp_path):
    m = _client(ctl, tmp_path)
    out, ref, est = _against_sklearn(m, tmp_path, GridSearchCV(Lasso(tol=1e-10, max_iter=100000),
                                                                {"alpha": [0.01, 0.1, 1.0]}, cv=3), ["alpha"])
    assert est.coef_.shape == (D_JOB,) and isinstance(est.intercept_, float) and est.n_iter_ >= 1
    assert est.dual_gap_ >= -1e-9 and est.model_type == "Lasso"
    assert np.abs(est.coef_ - ref.best_estimator_.coef_).max() <= 1e-7
    for r in out["job_result"]["results"]:
        assert len(r["n_iter"]) == 3 and all(i >= 1 for i in r["n_iter"])
    out, ref, est = _against_sklearn(
        m, tmp_path, GridSearchCV(ElasticNet(tol=1e-10, max_iter=100000),
                                  {"alpha": [0.01, 0.1, 1.0], "l1_ratio": [0.2, 0.8]}, cv=3), ["alpha", "l1_ratio"])
    assert est.model_type == "ElasticNet" and est.n_iter_ >= 1 and est.coef_.shape == (D_JOB,)
    with pytest.raises(AttributeError):
        est.feature_importances_


def test_ridge_job_matches_sklearn_cholesky(ctl, tmp_path):
    m = _client(ctl, tmp_path)
    grid = {"alpha": [0, 1e-3, 1, 1e3], "fit_intercept": [True, False]}
    out, ref, est = _against_sklearn(m, tmp_path, GridSearchCV(Ridge(solver="cholesky"), grid, cv=3),
                                     ["alpha", "fit_intercept"])
    assert est.model_type == "Ridge" and est.coef_.shape == (D_JOB,)
    with pytest.raises(AttributeError):
        est.n_iter_
    assert all("n_iter" not in r for r in out["job_result"]["results"])
    X, y = _job_table()
    worst = 0.0
    for a in grid["alpha"]:
        for fi in grid["fit_intercept"]:
            ours = refit_model({"model_type": "Ridge", "scoring": None}, {"alpha": a, "fit_intercept": fi},
                               DeviceData(X, y, False, "cpu"))
            skm = Ridge(alpha=a, fit_intercept=fi, solver="cholesky").fit(X.astype(np.float64), y.astype(np.float64))
            worst = max(worst, float(np.abs(ours["coef"] - skm.coef_).max() / np.abs(skm.coef_).max()))
            assert abs(ours["intercept"] - skm.intercept_) <= 1e-9
    print(f"Ridge vs sklearn cholesky: worst max|dcoef|/max|coef| = {worst:.3e}")
    assert worst <= 1e-9


# ---- edge cases ----------------------------------------------------------------------------------------
def _run(dd, model, params, **kw):
    kw.setdefault("holdout", False)
    return run_candidates(dd, JobSpec(model, params, cv=3, **kw), range(len(params)))


def test_column_constant_on_one_folds_training_rows():
    X, y = _job_table()
    X = X.copy()
    X[200:, 7] = 1.25          # KFold(3) without shuffling: fold 0 trains on rows 200..599
    dd = DeviceData(X, y, False, "cpu")
    for model, params in (("Lasso", {"alpha": 0.01}), ("ElasticNet", {"alpha": 0.01, "l1_ratio": 0.5}),
                          ("Ridge", {"alpha": 1.0}), ("Ridge", {"alpha": 0})):
        tasks, outs = _family_fits(dd, model, [params])
        by_split = {dd.split_names[t.split]: o for t, o in zip(tasks, outs)}
        tr0 = dd.train_rows[dd.split_names.index("cv0")].numpy()
        assert tr0.min() == 200 and len(tr0) == 400
        assert by_split["cv0"].model["coef"][7] == 0.0, (model, params)
        assert all(np.isfinite(o.model["coef"]).all() for o in outs)
        r = _run(dd, model, [params])[0]
        assert r.ok and np.isfinite(r.result["cv_scores"]).all() and min(r.result["cv_scores"]) > 0.5


def test_warnings_and_failed_candidates():
    X, y = _job_table()
    dd = DeviceData(X, y, False, "cpu")
    r = _run(dd, "Lasso", [{"alpha": 0.001, "max_iter": 2, "tol": 1e-12}])[0]
    assert r.ok and r.result["n_iter"] == [2, 2, 2]
    assert any(w.startswith("Objective did not converge (duality gap ") and w.endswith("increase max_iter")
               for w in r.result["warnings"]), r.result["warnings"]
    r = _run(dd, "Lasso", [{"alpha": 0}])[0]
    assert r.ok and linear.NO_L1 in r.result["warnings"]
    cyc, rnd = _run(dd, "ElasticNet", [{"alpha": 0.05}, {"alpha": 0.05, "selection": "random", "random_state": 3}])
    assert rnd.ok and linear.SELECTION_RANDOM in rnd.result["warnings"]
    assert "warnings" not in cyc.result and rnd.result["cv_scores"] == cyc.result["cv_scores"]
    bad = _run(dd, "Ridge", [{"alpha": 1.0, "positive": True}, {"alpha": 1.0}])
    assert not bad[0].ok and "ParamError" in bad[0].error and "positive" in bad[0].error and bad[1].ok
    bad = _run(dd, "ElasticNet", [{"l1_ratio": 1.5}, {"alpha": -1.0}, {"selection": "greedy"}, {"max_iter": 0}])
    assert all(not b.ok and "ParamError" in b.error for b in bad)
    assert "'l1_ratio' parameter of ElasticNet must be a float in the range [0.0, 1.0]" in bad[0].error
    r = _run(dd, "Lasso", [{"alpha": 0.1, "bogus": 1, "precompute": True, "warm_start": True, "copy_X": False}])[0]
    assert r.ok and r.result["warnings"] == ["ignored unknown parameters ['bogus']"]
    r = _run(dd, "Ridge", [{"alpha": 0.1, "solver": "sag", "tol": 1e-3, "max_iter": None, "random_state": 0}])[0]
    assert r.ok and "warnings" not in r.result


def test_registered_as_plain_regressors():
    fam = family_of("Lasso")
    assert fam is family_of("Ridge") is family_of("ElasticNet")
    assert {"Ridge", "Lasso", "ElasticNet"} <= set(supported_models())
    assert not fam.is_classifier("Lasso") and not getattr(fam, "self_scored", ()) and fam.data_parallel is False
    rp = fam.resolve("Lasso", {}, 1000, 50, 1)
    assert rp["l1_ratio"] == 1.0 and rp["max_iter"] == 1000 and rp["tol"] == 1e-4
    lin = family_of("LinearRegression")
    assert fam.cost("Lasso", rp, 10 ** 6, 100, 1) < lin.cost("LinearRegression", {}, 10 ** 6, 100, 1)


def test_multimetric_job_returns_both_labels():
    X, y = _job_table()
    dd = DeviceData(X, y, False, "cpu")
    pairs = [("r2", "r2"), ("neg_mean_squared_error", "neg_mean_squared_error")]
    res = _run(dd, "Lasso", [{"alpha": 0.01}, {"alpha": 0.5}], scoring=pairs, holdout=True)
    single = _run(dd, "Lasso", [{"alpha": 0.01}, {"alpha": 0.5}], scoring="neg_mean_squared_error", holdout=True)
    for r, s in zip(res, single):
        assert r.ok and list(r.result["scores"]) == ["r2", "neg_mean_squared_error"]
        assert r.result["scores"]["neg_mean_squared_error"]["cv_scores"] == pytest.approx(s.result["cv_scores"], rel=1e-12)
        assert r.result["scores"]["r2"]["holdout_score"] == pytest.approx(r.result["r2_score"], rel=1e-12)


def test_binned_only_table_streams_moments_and_test_rows(tmp_path):
    rng = np.random.RandomState(2)
    n, d = 3000, 9
    X = (rng.normal(size=(n, d)) + 2.0).astype(np.float32)
    y = (X @ rng.normal(size=d).astype(np.float32) + 3.0 + 0.2 * rng.normal(size=n)).astype(np.float32)
    mm = np.lib.format.open_memmap(str(tmp_path / "X.npy"), mode="w+", dtype=np.float32, shape=X.shape)
    mm[:] = X
    mm.flush()
    Xmm = np.load(str(tmp_path / "X.npy"), mmap_mode="r")
    res = DeviceData(X, y, False, "cpu")
    binned = DeviceData(Xmm, y, False, "cpu", binned_only=True, chunk_rows=700)
    assert binned.X is None and binned.can_stream_rows()
    for model, grid in (("Lasso", [{"alpha": 0.05, "tol": 1e-10, "max_iter": 100000}, {"alpha": 0.5, "fit_intercept": False}]),
                        ("Ridge", [{"alpha": 0.0}, {"alpha": 10.0, "fit_intercept": False}])):
        a = [r.result["cv_scores"] for r in _run(res, model, grid, holdout=True)]
        b = [r.result["cv_scores"] for r in _run(binned, model, grid, holdout=True)]
        np.testing.assert_allclose(np.asarray(b), np.asarray(a), rtol=0, atol=1e-8)

"""Multi-metric ``scoring`` (a list, tuple or dict of scorer names; docs/MULTIMETRIC.md) on the CPU
data path: the job through the client, ``score_from_stats`` against ``scoring.score`` and
``sklearn.metrics``, the host twin of the statistics kernel against numpy, the option errors, and
that a single-metric job runs none of it.

Tables: 300 rows and 6 features as in test_forest_permutation.py.  The regression target has mean
about 1 and standard deviation about 1, so sum y^2 / ss_tot stays below 10 (the amplification of
r2 computed from sums) and every target stays above -1 (the log errors' domain).

Tolerances.  A float64 sum of n = 100 held-out terms is good to about n * eps = 2e-14 relative,
times the amplification below 10: sum-based regression scores are compared at rtol = 1e-10, three
orders of margin.  Count-based scores are compared with ``==``."""
import json

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.engine import jobs
from cs230_distributed_machine_learning_amd.engine.service import Controller, job_plan
from cs230_distributed_machine_learning_amd.search import scoring

sk = pytest.importorskip("sklearn")
from sklearn import metrics as skm  # noqa: E402
from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor  # noqa: E402
from sklearn.model_selection import GridSearchCV  # noqa: E402

N, D = 300, 6
CLS_METRICS = ["accuracy", "f1_macro", "balanced_accuracy", "matthews_corrcoef"]
REG_METRICS = {"r2": "r2", "rmse": "neg_root_mean_squared_error", "mae": "neg_mean_absolute_error",
               "medae": "neg_median_absolute_error"}
ENTRY_KEYS = ("cv_scores", "mean_cv_score", "std_cv_score", "holdout_score")


def _table(is_cls):
    rng = np.random.RandomState(5)
    X = rng.normal(size=(N, D)).astype(np.float32)
    X[:, 5] = 1.0
    z = 2.0 * X[:, 0] - X[:, 1] + 0.1 * rng.normal(size=N)
    if is_cls:
        return X, np.searchsorted(np.quantile(z, [1 / 3, 2 / 3]), z).astype(np.int64)   # C = 3
    z = 1.0 + (z - z.mean()) / z.std()                    # mean 1, standard deviation 1
    return X, np.clip(z, -0.9, None).astype(np.float32)   # every target above -1


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
    return m


def _train(m, est, **extra):
    return m.train(est, "toy", {"target_column": "target", **extra}, wait_for_completion=True, polling_interval=0.02)


def _search(is_cls, scoring_opt, refit=True, **kw):
    base = RandomForestClassifier(n_estimators=5, random_state=0) if is_cls else \
        RandomForestRegressor(n_estimators=5, random_state=0)
    return GridSearchCV(base, {"max_depth": [2, None]}, cv=3, scoring=scoring_opt, refit=refit, **kw)


def _sk_ranks(means):
    """sklearn _format_results: rankdata(-mean, method="min"), NaN means as nanmin - 1 first."""
    from scipy.stats import rankdata

    v = np.array([np.nan if m is None else m for m in means], dtype=np.float64)
    if np.isnan(v).all():
        return [1] * len(v)
    v = np.where(np.isnan(v), np.nanmin(v) - 1, v)
    return [int(r) for r in rankdata(-v, method="min")]


def _by_params(results):
    return {json.dumps(r["parameters"], sort_keys=True): r for r in results}


# ---- 1, 2: the job -------------------------------------------------------------------------------
def test_classifier_job_equals_single_metric_jobs(ctl, tmp_path):
    m = _client(ctl, tmp_path, True)
    out = _train(m, _search(True, CLS_METRICS, refit="f1_macro"))
    assert out["job_status"] == "completed", out
    res = out["job_result"]["results"]
    assert len(res) == 2
    for r in res:
        assert list(r["scores"]) == CLS_METRICS
        assert r["scoring"] == "f1_macro"
        assert r["mean_cv_score"] == r["scores"]["f1_macro"]["mean_cv_score"]
        assert r["cv_scores"] == r["scores"]["f1_macro"]["cv_scores"]
        assert r["std_cv_score"] == r["scores"]["f1_macro"]["std_cv_score"]
        assert r["scores"]["accuracy"]["holdout_score"] == r["accuracy"]
        assert all(e["scorer"] == label and set(ENTRY_KEYS) <= set(e) for label, e in r["scores"].items())
    multi = _by_params(res)
    for name in CLS_METRICS:   # the same trees (random_state), the same folds: the same bits
        single = _train(m, _search(True, name))
        assert single["job_status"] == "completed", single
        for key, s in _by_params(single["job_result"]["results"]).items():
            e = multi[key]["scores"][name]
            assert "scores" not in s
            assert e["cv_scores"] == s["cv_scores"], name
            assert e["mean_cv_score"] == s["mean_cv_score"] and e["std_cv_score"] == s["std_cv_score"], name
            assert multi[key]["accuracy"] == s["accuracy"]
    means = [r["scores"]["f1_macro"]["mean_cv_score"] for r in res]
    assert out["job_result"]["best_result"]["parameters"] == res[int(np.argmax(means))]["parameters"]
    mm = out["job_result"]["multimetric"]
    assert mm["scoring"] == {n: n for n in CLS_METRICS} and mm["refit"] == "f1_macro"
    for name in CLS_METRICS:
        assert mm["rank_test"][name] == _sk_ranks([r["scores"][name]["mean_cv_score"] for r in res])
    assert out["job_result"]["best_result"].get("model_path")   # refitted like refit=True


def test_regressor_job_dict_labels(ctl, tmp_path):
    m = _client(ctl, tmp_path, False)
    out = _train(m, _search(False, REG_METRICS, refit="rmse"))
    assert out["job_status"] == "completed", out
    res = out["job_result"]["results"]
    for r in res:
        assert list(r["scores"]) == list(REG_METRICS)           # the labels as given, in order
        assert [e["scorer"] for e in r["scores"].values()] == list(REG_METRICS.values())
        assert r["scoring"] == "neg_root_mean_squared_error"
        assert r["mean_cv_score"] == r["scores"]["rmse"]["mean_cv_score"]
    multi = _by_params(res)
    worst = 0.0
    for label, name in REG_METRICS.items():
        single = _train(m, _search(False, name))
        assert single["job_status"] == "completed", single
        for key, s in _by_params(single["job_result"]["results"]).items():
            e = multi[key]["scores"][label]
            if label == "medae":   # not a function of the sums: the per-fit path, the same code
                assert e["cv_scores"] == s["cv_scores"] and e["mean_cv_score"] == s["mean_cv_score"]
                continue
            a, b = np.array(e["cv_scores"] + [e["mean_cv_score"]]), np.array(s["cv_scores"] + [s["mean_cv_score"]])
            worst = max(worst, float(np.max(np.abs(a - b) / np.abs(b))))
            np.testing.assert_allclose(a, b, rtol=1e-10, atol=0)
    print("largest relative difference, statistics route vs per-fit route:", worst)
    means = [r["scores"]["rmse"]["mean_cv_score"] for r in res]
    assert out["job_result"]["best_result"]["parameters"] == res[int(np.argmax(means))]["parameters"]
    mm = out["job_result"]["multimetric"]
    assert mm["scoring"] == REG_METRICS and mm["refit"] == "rmse"
    assert all(mm["rank_test"][lb] == _sk_ranks([r["scores"][lb]["mean_cv_score"] for r in res]) for lb in REG_METRICS)


# ---- 3: score_from_stats -------------------------------------------------------------------------
def _cls_case(C, seed, n=211):
    """Random labels, half of them right.  C > 2: class C - 1 is never true and class 0 is never
    predicted (an empty row and an empty column of the confusion matrix)."""
    rng = np.random.RandomState(seed)
    if C == 2:
        y, p = rng.randint(0, 2, size=n), rng.randint(0, 2, size=n)
    else:
        y, p = rng.randint(0, C - 1, size=n), rng.randint(1, C, size=n)
    agree = (rng.rand(n) < 0.5) & (y >= (0 if C == 2 else 1))
    return y.astype(np.int32), np.where(agree, y, p).astype(np.int32)


def _sk_cls(name, y, p, C):
    labels = list(range(C))
    for what, fn in (("precision", skm.precision_score), ("recall", skm.recall_score), ("f1", skm.f1_score),
                     ("jaccard", skm.jaccard_score)):
        if name == what:
            return fn(y, p, zero_division=0)
        if name.startswith(what + "_"):
            return fn(y, p, average=name.split("_", 1)[1], labels=labels, zero_division=0)
    if name == "accuracy":
        return skm.accuracy_score(y, p)
    if name == "balanced_accuracy":
        return skm.balanced_accuracy_score(y, p)
    if name == "matthews_corrcoef":
        return skm.matthews_corrcoef(y, p)
    if name == "positive_likelihood_ratio":
        return skm.class_likelihood_ratios(y, p)[0]
    if name == "neg_negative_likelihood_ratio":
        return -skm.class_likelihood_ratios(y, p)[1]
    return getattr(skm, name)(y, p)


@pytest.mark.parametrize("C", [2, 3, 7])
def test_classification_scores_from_stats(C):
    import warnings

    y, p = _cls_case(C, 10 + C)
    if C > 2:
        assert (C - 1) not in y and 0 not in p
    off = np.array([0, len(y)], dtype=np.int64)
    rows = torch.arange(len(y), dtype=torch.int32)
    cm = scoring.fit_statistics(rows, off, torch.from_numpy(p), torch.from_numpy(y), C)[0]
    np.testing.assert_array_equal(cm, skm.confusion_matrix(y, p, labels=list(range(C))))
    seen = 0
    for name in scoring.CLS_STAT_SCORERS:
        binary = name in ("precision", "recall", "f1", "jaccard", "positive_likelihood_ratio",
                          "neg_negative_likelihood_ratio")
        if binary and C != 2:
            with pytest.raises(ValueError, match="binary"):
                scoring.score_from_stats(name, cm, C)
            continue
        got = scoring.score_from_stats(name, cm, C)
        assert got == scoring.score(name, torch.from_numpy(y), torch.from_numpy(p), C), name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = float(_sk_cls(name, y, p, C))
        assert abs(got - ref) <= 1e-12, (name, got, ref)
        seen += 1
    assert seen == len(scoring.CLS_STAT_SCORERS) - (0 if C == 2 else 6)


def _reg_case(seed, n=157):
    rng = np.random.RandomState(seed)
    y = (1.0 + rng.normal(size=n)).astype(np.float32)
    y = np.clip(y, 0.05, None)                                    # strictly positive: every domain holds
    p = np.clip(y + 0.3 * rng.normal(size=n), 0.05, None).astype(np.float32)
    return y, p


def _sk_reg(name, y, p):
    return {
        "r2": lambda: skm.r2_score(y, p),
        "neg_mean_squared_error": lambda: -skm.mean_squared_error(y, p),
        "neg_root_mean_squared_error": lambda: -np.sqrt(skm.mean_squared_error(y, p)),
        "neg_mean_absolute_error": lambda: -skm.mean_absolute_error(y, p),
        "explained_variance": lambda: skm.explained_variance_score(y, p),
        "max_error": lambda: -skm.max_error(y, p),
        "neg_max_error": lambda: -skm.max_error(y, p),
        "neg_mean_absolute_percentage_error": lambda: -skm.mean_absolute_percentage_error(y, p),
        "neg_mean_squared_log_error": lambda: -skm.mean_squared_log_error(y, p),
        "neg_root_mean_squared_log_error": lambda: -np.sqrt(skm.mean_squared_log_error(y, p)),
        "neg_mean_poisson_deviance": lambda: -skm.mean_poisson_deviance(y, p),
        "neg_mean_gamma_deviance": lambda: -skm.mean_gamma_deviance(y, p),
    }[name]()


def test_regression_scores_from_stats():
    y, p = _reg_case(3)
    off = np.array([0, len(y)], dtype=np.int64)
    rows = torch.arange(len(y), dtype=torch.int32)
    st = scoring.fit_statistics(rows, off, torch.from_numpy(p), torch.from_numpy(y), 0,
                                want=scoring.stats_want(scoring.REG_STAT_SCORERS))[0]
    assert scoring.stats_want(scoring.REG_STAT_SCORERS) == 7 and scoring.stats_want(["r2", "max_error"]) == 0
    y64, p64 = y.astype(np.float64), p.astype(np.float64)   # the float32 arrays, widened
    worst = 0.0
    for name in scoring.REG_STAT_SCORERS:
        got, ref = scoring.score_from_stats(name, st), float(_sk_reg(name, y64, p64))
        worst = max(worst, abs(got - ref) / abs(ref))
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=0, err_msg=name)
        np.testing.assert_allclose(got, scoring.score(name, torch.from_numpy(y), torch.from_numpy(p)), rtol=1e-10,
                                   atol=0, err_msg=name)
    print("largest relative difference to sklearn.metrics:", worst)
    assert set(scoring.CLS_STAT_SCORERS) | set(scoring.REG_STAT_SCORERS) == set(scoring.STAT_SCORERS)
    assert not scoring.STAT_SCORERS & {"neg_median_absolute_error", "d2_absolute_error_score", *scoring.PROBA_SCORERS}


@pytest.mark.parametrize("name,ybad,pbad,message", [
    ("neg_mean_squared_log_error", -1.0, None, "Mean Squared Logarithmic Error cannot be used"),
    ("neg_mean_poisson_deviance", None, 0.0, "power=1 can only be used on non-negative y"),
    ("neg_mean_gamma_deviance", 0.0, None, "power=2 can only be used on strictly positive y"),
])
def test_invalid_domain_raises_like_score(name, ybad, pbad, message):
    y, p = _reg_case(4)
    if ybad is not None:
        y[11] = ybad
    if pbad is not None:
        p[11] = pbad
    off = np.array([0, len(y)], dtype=np.int64)
    st = scoring.fit_statistics(torch.arange(len(y), dtype=torch.int32), off, torch.from_numpy(p), torch.from_numpy(y),
                                0, want=7)[0]
    with pytest.raises(ValueError, match=message):
        scoring.score_from_stats(name, st)
    with pytest.raises(ValueError, match=message):
        scoring.score(name, torch.from_numpy(y), torch.from_numpy(p))
    assert np.isfinite(scoring.score_from_stats("r2", st))   # the other scorers are not affected


# ---- 4: the host twin ------------------------------------------------------------------------------
LENS = (0, 1, 255, 256, 257, 600)


def _concat_case(C, seed, n=5000):
    rng = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    rows = rng.randint(0, n, size=off[-1]).astype(np.int32)    # scattered over the target vector
    if C:
        return off, rows, rng.randint(0, C, size=off[-1]).astype(np.int32), rng.randint(0, C, size=n).astype(np.int32)
    y = (1.0 + rng.normal(size=n)).astype(np.float32)
    return off, rows, (y[rows] + 0.5 * rng.normal(size=off[-1])).astype(np.float32), y


@pytest.mark.parametrize("C", [2, 3, 5, 64, 65])
def test_host_twin_confusion_matrices(C):
    off, rows, p, y = _concat_case(C, C)
    cm = scoring.fit_statistics(torch.from_numpy(rows), off, torch.from_numpy(p), torch.from_numpy(y), C)
    assert cm.shape == (len(LENS), C, C) and cm.dtype == np.int64
    for f in range(len(LENS)):
        sl = slice(off[f], off[f + 1])
        ref = np.bincount(y[rows[sl]].astype(np.int64) * C + p[sl], minlength=C * C).reshape(C, C)
        np.testing.assert_array_equal(cm[f], ref)
    bad = p.copy()
    bad[off[4] + 3] = C   # one prediction outside [0, C)
    with pytest.raises(ValueError, match=r"fit 4 has 1 prediction"):
        scoring.fit_statistics(torch.from_numpy(rows), off, torch.from_numpy(bad), torch.from_numpy(y), C)


def test_host_twin_regression_sums():
    off, rows, p, y = _concat_case(0, 9)
    args = (torch.from_numpy(rows), off, torch.from_numpy(p), torch.from_numpy(y), 0)
    st = scoring.fit_statistics(*args, want=7)
    st0 = scoring.fit_statistics(*args, want=0)
    assert st.shape == (len(LENS), 14) and st.dtype == np.float64
    eps = np.finfo(np.float64).eps
    for f in range(len(LENS)):
        sl = slice(off[f], off[f + 1])
        yy, pp = y[rows[sl]].astype(np.float64), p[sl].astype(np.float64)
        e = pp - yy
        ok_log, ok_poi, ok_gam = (yy > -1) & (pp > -1), (yy >= 0) & (pp > 0), (yy > 0) & (pp > 0)
        with np.errstate(all="ignore"):
            xlogy = np.where(yy > 0, yy * np.log(np.where(ok_poi & (yy > 0), yy / pp, 1.0)), 0.0)
            ref = [len(yy), yy.sum(), (yy * yy).sum(), e.sum(), (e * e).sum(), np.abs(e).sum(),
                   np.abs(e).max() if len(yy) else 0.0, (np.abs(e) / np.maximum(np.abs(yy), eps)).sum(),
                   ((np.log1p(yy[ok_log]) - np.log1p(pp[ok_log])) ** 2).sum(), (~ok_log).sum(),
                   (2 * (xlogy - yy + pp))[ok_poi].sum(), (~ok_poi).sum(),
                   (2 * (np.log(pp[ok_gam] / yy[ok_gam]) + yy[ok_gam] / pp[ok_gam] - 1)).sum(), (~ok_gam).sum()]
        for j in (0, 6, 9, 11, 13):   # counts and the maximum: exact
            assert st[f, j] == ref[j], (f, j)
        for j in (1, 2, 3, 4, 5, 7, 8, 10, 12):
            # 1e-12 of the sum of the terms' magnitudes (slot 3 and the deviances add signed terms)
            mag = {3: np.abs(e).sum(), 10: np.abs(2 * (xlogy - yy + pp))[ok_poi].sum()}.get(j, abs(ref[j]))
            assert abs(st[f, j] - ref[j]) <= 1e-12 * mag, (f, j, st[f, j], ref[j])
    assert st[3, 11] > 0 and st[5, 13] > 0          # the case does leave the deviances' domain
    for j in range(14):                              # want = 0: the logarithm slots are 0, the rest unchanged
        np.testing.assert_array_equal(st0[:, j], 0.0 if j in (8, 10, 12) else st[:, j])
    with pytest.raises(ValueError, match="outside the target vector"):
        r2 = rows.copy()
        r2[off[2]] = len(y)
        scoring.fit_statistics(torch.from_numpy(r2), off, torch.from_numpy(p), torch.from_numpy(y), 0)


# ---- 5: option errors ------------------------------------------------------------------------------
def _f1(y, p):
    return 0.0


@pytest.mark.parametrize("is_cls,scoring_opt,refit,message", [
    (True, ["accuracy", "f1_macro"], True, "refit must be set to a scorer key or False"),
    (True, ["accuracy", "f1_macro"], "recall_macro", "'recall_macro' is not one of the scorer keys"),
    (True, ["accuracy", "accuracy"], "accuracy", "must be unique"),
    (True, [], False, "an empty list gives no metric"),
    (True, {"mine": _f1}, "mine", "callables are not supported"),
    (True, ["accuracy", _f1], "accuracy", "callables are not supported"),
    (False, ["r2", "accuracy"], "r2", "scoring 'accuracy' not supported for this estimator"),
])
def test_option_errors(ctl, tmp_path, is_cls, scoring_opt, refit, message):
    m = _client(ctl, tmp_path, is_cls)
    out = _train(m, _search(is_cls, scoring_opt, refit=refit))
    assert out.get("status") == "error" and out.get("code") == 400 and message in out["message"], out


def test_plan_forms():
    from cs230_distributed_machine_learning_amd.models.base import ParamError

    def plan(model, scoring_opt, refit):
        return job_plan({"model_details": {"model_type": model, "search_type": "GridSearchCV", "hyperparameters": {
            "search_params": {"param_grid": {"max_depth": [2]}}, "cv_params": {"cv": 3, "scoring": scoring_opt,
                                                                               "refit": refit}}}})

    p = plan("RandomForestClassifier", ("accuracy", "f1_macro"), "f1_macro")   # a tuple is a list
    assert p["scoring_labels"] == ["accuracy", "f1_macro"] and p["scoring_names"] == ["accuracy", "f1_macro"]
    assert p["refit_metric"] == "f1_macro" and p["scoring"] == "f1_macro" and p["refit"] is True
    p = plan("RandomForestClassifier", {"a": "accuracy", "b": "recall_macro"}, False)
    assert p["refit_metric"] == "a" and p["scoring"] == "accuracy" and p["refit"] is False
    p = plan("RandomForestClassifier", "f1_macro", True)
    assert not [k for k in p if k in ("scoring_labels", "scoring_names", "refit_metric")]
    for bad in ({"accuracy"}, 3):
        with pytest.raises(ParamError, match="a scorer name, a non-empty list or tuple"):
            plan("RandomForestClassifier", bad, False)
    with pytest.raises(ParamError, match="needs predictions; PCA only has score"):
        plan("PCA", ["accuracy"], False)


def test_client_wire_forms():
    from distributed_ml import MLTaskManager

    enc = MLTaskManager._extract_model_details
    for form in (["accuracy", "f1_macro"], ("accuracy", "f1_macro"), {"a": "accuracy", "b": "f1_macro"}):
        d = enc(None, _search(True, form, refit=False))
        wire = json.loads(json.dumps(d, default=MLTaskManager._json_serializer))
        got = wire["hyperparameters"]["cv_params"]["scoring"]
        assert got == (form if isinstance(form, dict) else list(form))
        assert list(got) == list(form)   # a dict keeps its order


# ---- 6: a single-metric job runs none of it -------------------------------------------------------
def test_string_scoring_job_runs_none_of_it(ctl, tmp_path, monkeypatch):
    calls = []
    real = scoring.fit_statistics
    monkeypatch.setattr(scoring, "fit_statistics", lambda *a, **k: calls.append(1) or real(*a, **k))
    m = _client(ctl, tmp_path, True)
    for opt in ("f1_macro", None):
        out = _train(m, _search(True, opt))
        assert out["job_status"] == "completed", out
        assert all("scores" not in r for r in out["job_result"]["results"])
        assert "multimetric" not in out["job_result"]
    assert not calls
    out = _train(m, _search(True, ["accuracy", "f1_macro"], refit=False))   # the spy does see a multi-metric job
    assert out["job_status"] == "completed" and calls


# ---- 7: refit=False ----------------------------------------------------------------------------------
def test_refit_false_first_label_is_primary(ctl, tmp_path):
    m = _client(ctl, tmp_path, True)
    out = _train(m, _search(True, ["balanced_accuracy", "accuracy"], refit=False))
    assert out["job_status"] == "completed", out
    res = out["job_result"]["results"]
    for r in res:
        assert r["scoring"] == "balanced_accuracy"
        assert r["mean_cv_score"] == r["scores"]["balanced_accuracy"]["mean_cv_score"]
        assert not r.get("model_path")   # no refit model
    mm = out["job_result"]["multimetric"]
    assert mm["refit"] is False and sorted(mm["rank_test"]) == ["accuracy", "balanced_accuracy"]
    assert all(sorted(v)[0] == 1 and len(v) == len(res) for v in mm["rank_test"].values())


def test_rank_rule():
    assert jobs.rank_test([0.5, None, 0.7, 0.5]) == [2, 4, 1, 2] == _sk_ranks([0.5, None, 0.7, 0.5])
    assert jobs.rank_test([None, float("nan")]) == [1, 1]
    assert jobs.rank_test([]) == []


# ---- 8: journal replay -----------------------------------------------------------------------------
def test_journal_replay_keeps_the_new_keys(tmp_path):
    cfg = dict(data_root=str(tmp_path / "data"), journal=str(tmp_path / "journal.jsonl"), device="cpu",
               sse_interval_s=0.05)
    c = Controller(Config(**cfg))
    try:
        m = _client(c, tmp_path, True)
        out = _train(m, _search(True, CLS_METRICS, refit="f1_macro"))
        assert out["job_status"] == "completed", out
        sid, jid = m.session_id, m.job_id
    finally:
        c.shutdown()
    c2 = Controller(Config(**cfg))
    try:
        status, again = c2.check_status(sid, jid)
        assert status == 200 and again["job_status"] == "completed"
        assert again["job_result"]["multimetric"] == out["job_result"]["multimetric"]
        before, after = out["job_result"]["results"], again["job_result"]["results"]
        assert [r["scores"] for r in after] == [r["scores"] for r in before]
    finally:
        c2.shutdown()

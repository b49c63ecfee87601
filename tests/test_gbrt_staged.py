"""GradientBoosting per-stage statistics (docs/GBRT_STAGED.md) on the CPU data path: the
statistics op (csrc/runtime/gbrt_stats_cpu.cpp, the twin of gbrt.hip k_gb_stage_stats) against a
float64 reference built from sklearn's own loss classes, the kept model's ``train_score_`` /
``feature_importances_`` / staged predictions against sklearn on exactly binned data, the
out-of-bag recurrences, and ``train_params["staged_scores"]`` end to end through the client.
"""
import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.model_store import Predictor, load_model, save_model
from cs230_distributed_machine_learning_amd.engine.service import Controller
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.ops import gbrt_ops

pytest.importorskip("sklearn")
from sklearn._loss.loss import (AbsoluteError, ExponentialLoss, HalfBinomialLoss, HalfMultinomialLoss,  # noqa: E402
                                HalfSquaredError, HuberLoss, PinballLoss)
from sklearn.datasets import make_classification  # noqa: E402
from sklearn.ensemble import GradientBoostingClassifier, GradientBoostingRegressor  # noqa: E402
from sklearn.model_selection import GridSearchCV  # noqa: E402

from gbrt_stage_cases import ABS, CLS_MIX, EXP, HUBER, LOG, QUANT, REG_MIX, SQ, categories, make_case, run_case  # noqa: E402

CLS, REG = "GradientBoostingClassifier", "GradientBoostingRegressor"
# float64 sums added in another order, non-negative terms each good to a few ulp
SUM_RTOL = 1e-12
# largest deviations from sklearn measured on the CPU path over the four binned cases below
# (docs/GBRT_STAGED.md): train_score_ 2.8e-9 relative, feature_importances_ 3.6e-9 absolute;
# the tests allow ten times that
TRAIN_SCORE_RTOL = 2.8e-8
IMPORTANCES_ATOL = 3.6e-8
# raw scores: the project's parity claim for classifiers; a regressor's stage trees are grown on
# float32 residuals (eps 6e-8, |residual| < 40 here), which its leaf means inherit
RAW_ATOL = {True: 1e-9, False: 1e-6}


# ---- the op against sklearn's loss classes ----------------------------------------------------
def _reference(c):
    """Per fit and category: (n, match count or SSE, loss sum) in float64 numpy."""
    F, K, n = c["F"], c["K"], c["n"]
    out = []
    for f in range(F):
        raw = c["raw"][f * K:(f + 1) * K]
        loss = int(c["loss"][f])
        row = []
        for m in categories(c, f):
            y = c["y"][m]
            r = np.ascontiguousarray(raw[:, m].T)                      # [m, K]
            if loss == LOG and K > 1:
                obj, rp, stat = HalfMultinomialLoss(n_classes=K), r, int((r.argmax(1) == y).sum())
            elif loss in (LOG, EXP):
                obj = HalfBinomialLoss() if loss == LOG else ExponentialLoss()
                rp, stat = r[:, 0].copy(), int(((r[:, 0] >= 0).astype(int) == y).sum())
            else:
                obj = {SQ: HalfSquaredError(), ABS: AbsoluteError(), QUANT: PinballLoss(quantile=float(c["alpha"][f])),
                       HUBER: HuberLoss(quantile=0.9, delta=float(c["delta"][f]))}[loss]
                rp, stat = r[:, 0].copy(), float(((r[:, 0] - y) ** 2).sum())
            ls = float(obj.loss(y_true=y.astype(np.float64), raw_prediction=rp).sum()) if m.any() else 0.0
            row.append((int(m.sum()), stat, ls))
        out.append(row)
    return out


def _check(c, stats, stage=1):
    cnt, stat, lsum = gbrt_ops.stats_arrays(stats[:, stage], c["is_cls"])
    assert np.isfinite(lsum).all() and not np.isnan(np.asarray(stat, dtype=np.float64)).any()
    for f, row in enumerate(_reference(c)):
        for k, (n_ref, stat_ref, loss_ref) in enumerate(row):
            assert cnt[f, k] == n_ref, (f, k)
            if c["is_cls"]:
                assert stat[f, k] == stat_ref, (f, k)
            else:
                assert stat[f, k] == pytest.approx(stat_ref, rel=SUM_RTOL, abs=0.0), (f, k)
            assert lsum[f, k] == pytest.approx(loss_ref, rel=SUM_RTOL, abs=0.0), (f, k, lsum[f, k], loss_ref)
    untouched = np.delete(stats, stage, axis=1)
    assert not untouched.any()                                          # only the destination stage is written


@pytest.mark.parametrize("n", [1, 256, 257, 300])
@pytest.mark.parametrize("losses,K", [(CLS_MIX, 1), ([LOG] * 5, 3), ([LOG] * 5, 9), (REG_MIX, 1), ([EXP], 1),
                                      ([LOG], 1), ([LOG], 3), ([SQ], 1), ([ABS], 1), ([HUBER], 1), ([QUANT], 1)])
def test_stats_equal_the_sklearn_losses(n, losses, K):
    c = make_case(n, K, losses, seed=n + K)
    stats, _part = run_case(c, "cpu")
    _check(c, stats)


@pytest.mark.parametrize("losses,K", [(CLS_MIX, 1), ([LOG] * 2, 3), ([LOG], 9), (REG_MIX, 1)])
@pytest.mark.parametrize("mode", ["big", "ties"])
def test_large_scores_and_exact_ties(losses, K, mode):
    c = make_case(300, K, losses, seed=7, mode=mode)
    if mode == "ties" and K == 1 and c["is_cls"]:
        assert (c["raw"] == 0.0).any()                                  # raw exactly 0 predicts class 1
    if mode == "ties" and K > 1:
        top = c["raw"].reshape(c["F"], K, -1)
        assert ((top == top.max(1, keepdims=True)).sum(1) > 1).any()    # exact ties: the first maximum wins
    stats, _part = run_case(c, "cpu")
    _check(c, stats)


def test_empty_categories_and_no_validation_mask():
    c = make_case(300, 1, CLS_MIX, seed=3, empty_oob=True, with_val=False)
    stats, _part = run_case(c, "cpu")
    _check(c, stats)
    cnt, _stat, lsum = gbrt_ops.stats_arrays(stats[:, 1], True)
    assert not cnt[:, 1].any() and not lsum[:, 1].any()
    curves = gbrt_ops.stage_curves(stats[0], LOG, 1)
    assert np.isnan(curves["oob_loss"]).all() and np.isnan(curves["train_loss"][0])   # stage 0 was never written


def test_partials_add_up_in_block_order_and_runs_repeat():
    c = make_case(300, 1, REG_MIX, seed=11)
    stats, part = run_case(c, "cpu")
    stats2, part2 = run_case(c, "cpu")
    assert stats.tobytes() == stats2.tobytes() and part.tobytes() == part2.tobytes()
    assert part.shape[0] == 2
    sse = part[..., 1].copy().view(np.float64)
    assert ((sse[0] + sse[1]).view(np.int64) == stats[:, 1, :, 1]).all()
    assert (part[..., 0].sum(0) == stats[:, 1, :, 0]).all()


@pytest.mark.parametrize("n", [16 * 256 + 1, 256 * 256 + 1])
def test_reduction_levels(n):
    """17 blocks are two levels of the 16-to-1 reduction, 257 blocks three."""
    for losses in ([LOG, EXP], [SQ, HUBER]):
        c = make_case(n, 1, losses, seed=5)
        stats, part = run_case(c, "cpu")
        _check(c, stats)
        assert (part[..., 0].sum(0) == stats[:, 1, :, 0]).all()


def test_plan_rejects_indices_outside_their_arrays():
    ok = dict(K=1, raw_rows=2, role_rows=1, inbag_rows=2, val_rows=0, stat_fits=2, delta_len=2, device="cpu")
    z = [0, 1]
    gbrt_ops.stats_plan(z, [SQ, SQ], [0, 0], z, [-1, -1], z, z, [0.5, 0.5], **ok)
    for bad in range(7):
        cols = [z, [SQ, SQ], [0, 0], z, [-1, -1], z, z]
        cols[bad] = [0, 7]
        with pytest.raises(ValueError, match="out of range"):
            gbrt_ops.stats_plan(*cols, [0.5, 0.5], **ok)


def test_stage_curves_formulas():
    st = np.zeros((2, 3, 3), np.int64)
    f64 = lambda v: np.float64(v).view(np.int64)   # noqa: E731
    st[1, 0] = (4, f64(2.0), f64(6.0))
    st[1, 2] = (5, f64(10.0), f64(1.0))
    for name, want in (("r2", 1 - 10.0 / 40.0), ("neg_mean_squared_error", -2.0),
                       ("neg_root_mean_squared_error", -np.sqrt(2.0))):
        c = gbrt_ops.stage_curves(st, SQ, 1, name, ss_tot=40.0)
        assert c["test_score"][1] == want and c["train_loss"][1] == 2 * 6.0 / 4 and c["test_loss"][1] == 2 * 1.0 / 5
    assert gbrt_ops.stage_curves(st, ABS, 1, None, ss_tot=40.0)["train_loss"][1] == 6.0 / 4
    st[1, 2, 1] = 3
    c = gbrt_ops.stage_curves(st, LOG, 3)
    assert c["test_score"][1] == 3 / 5 and c["scoring"] == "accuracy" and c["test_loss"][1] == 1.0 / 5
    assert gbrt_ops.stage_curves(st, LOG, 1)["test_loss"][1] == 2 * 1.0 / 5
    with pytest.raises(ValueError, match="accuracy"):
        gbrt_ops.stage_curves(st, LOG, 1, "r2")


# ---- kept models against sklearn on exactly binned data ---------------------------------------
N, D = 400, 6


def _binned(n_classes, seed=1):
    """400 x 6, at most 32 distinct values per feature: the 256-bin thresholds are exact."""
    X, y = make_classification(N, D, n_informative=4, n_redundant=0, n_classes=max(2, n_classes), random_state=3)
    X = np.floor((X - X.min(0)) / (X.max(0) - X.min(0)) * 31.999).astype(np.float32)
    if n_classes == 0:
        rng = np.random.RandomState(seed)
        y = (X[:, 0] - 0.5 * X[:, 1] + 0.02 * X[:, 2] * X[:, 3] + 3.0 * rng.normal(size=N)).astype(np.float32)
    return X, y


def _fit(name, X, y, params, staged=None, split_roles=None, want_masks=False):
    is_cls = name == CLS
    dd = DeviceData(X, y, is_cls, "cpu")
    dd.set_splits(np.ones((1, len(y)), np.uint8) if split_roles is None else split_roles, ["full"])
    fam = family_of(name)
    rp = fam.resolve(name, params, dd.train_counts[0], X.shape[1], dd.n_classes)
    task = FitTask(0, 0, 0, name, rp, staged=staged)
    K = dd.n_classes if (is_cls and dd.n_classes > 2) else 1
    if want_masks:
        return fam._boost(dd, [task], K, True, want_masks=True)[0]
    return fam.run(dd, [task], keep_models=True)[0]


CASES = [(CLS, 2, {}, 1), (CLS, 3, {}, 1), (REG, 0, {"loss": "squared_error"}, 1), (REG, 0, {"loss": "huber"}, 1)]
_sk_cache = {}


def _pair(i):
    """(Predictor of the kept fit, the fitted sklearn estimator, X, y) of CASES[i], made once."""
    if i not in _sk_cache:
        name, n_classes, extra, seed = CASES[i]
        X, y = _binned(n_classes, seed)
        # leaves of at least 8 rows: a split that cuts off one or two rows of a small node is often
        # the same cut on several features, and sklearn's feature order then credits another one
        params = {"n_estimators": 10, "max_depth": 3, "min_samples_leaf": 8, "random_state": 3, **extra}
        out = _fit(name, X, y, params)
        sk = (GradientBoostingClassifier if name == CLS else GradientBoostingRegressor)(**params)
        _sk_cache[i] = (Predictor(out.model), sk.fit(X, y.astype(np.float64) if name == REG else y), X, y)
    return _sk_cache[i]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_train_score_is_sklearns(i):
    pr, sk, _X, _y = _pair(i)
    dev = np.max(np.abs(pr.train_score_ - sk.train_score_) / np.abs(sk.train_score_))
    print(f"train_score_ relative deviation {dev:.3e}")
    assert pr.train_score_.shape == (10,) and pr.n_estimators_ == 10
    np.testing.assert_allclose(pr.train_score_, sk.train_score_, rtol=TRAIN_SCORE_RTOL, atol=0.0)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_feature_importances_are_sklearns(i):
    pr, sk, _X, _y = _pair(i)
    dev = np.max(np.abs(pr.feature_importances_ - sk.feature_importances_))
    print(f"feature_importances_ absolute deviation {dev:.3e}")
    assert pr.feature_importances_.sum() == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_allclose(pr.feature_importances_, sk.feature_importances_, rtol=0.0, atol=IMPORTANCES_ATOL)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_staged_predictions_are_sklearns(i):
    pr, sk, X, _y = _pair(i)
    ours, ref = list(pr.staged_predict(X)), list(sk.staged_predict(X))
    raws = list(pr.staged_decision_function(X))
    raw_ref = list(sk.staged_decision_function(X)) if pr.is_classifier else [p[:, None] for p in ref]
    assert len(ours) == len(ref) == len(raws) == 10
    for s in range(10):
        np.testing.assert_allclose(raws[s], raw_ref[s].reshape(raws[s].shape), rtol=0.0, atol=RAW_ATOL[pr.is_classifier])
        if pr.is_classifier:
            r = raw_ref[s].reshape(len(X), -1)
            top = np.sort(r, 1)
            clear = np.abs(r[:, 0]) > 1e-6 if r.shape[1] == 1 else top[:, -1] - top[:, -2] > 1e-6   # away from ties
            assert clear.mean() > 0.9 and (ours[s][clear] == ref[s][clear]).all()
        else:
            np.testing.assert_allclose(ours[s], ref[s], rtol=0.0, atol=RAW_ATOL[False])
    np.testing.assert_array_equal(ours[-1], pr.predict(X))
    if pr.is_classifier:
        np.testing.assert_allclose(list(pr.staged_predict_proba(X))[-1], sk.predict_proba(X), rtol=0.0, atol=1e-9)


def test_constant_target_has_zero_importances():
    X, _y = _binned(0)
    out = _fit(REG, X, np.ones(N, np.float32), {"n_estimators": 3, "random_state": 0})
    pr = Predictor(out.model)
    assert pr.feature_importances_.shape == (D,) and not pr.feature_importances_.any()


# ---- consistency ------------------------------------------------------------------------------
def _mean_loss(name, loss, raw, y):
    """factor * mean loss of sklearn's ``_fit_stages`` from raw scores [m, k], in numpy."""
    if name == CLS and raw.shape[1] == 1:
        z = raw[:, 0]
        return 2.0 * np.mean(np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - y * z)
    if name == CLS:
        mx = raw.max(1)
        return np.mean(mx + np.log(np.exp(raw - mx[:, None]).sum(1)) - raw[np.arange(len(y)), y])
    d = y.astype(np.float64) - raw[:, 0]
    return 2.0 * np.mean(0.5 * d * d)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_train_score_is_the_loss_of_the_staged_raw_scores(i):
    pr, _sk, X, y = _pair(i)
    ref = [_mean_loss(CASES[i][0], None, raw, y) for raw in pr.staged_decision_function(X)]
    np.testing.assert_allclose(pr.train_score_, ref, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name,n_classes", [(CLS, 2), (REG, 0)])
def test_out_of_bag_recurrences(name, n_classes):
    X, y = _binned(n_classes)
    out = _fit(name, X, y, {"n_estimators": 8, "subsample": 0.5, "random_state": 5}, want_masks=True)
    pr = Predictor(out.model)
    oob, imp = pr.oob_scores_, pr.oob_improvement_
    assert oob.shape == imp.shape == pr.train_score_.shape == (8,) and pr.oob_score_ == oob[-1]
    assert (imp[1:] == oob[:-1] - oob[1:]).all()                        # sklearn's recurrence, exactly
    # the curves are the losses of the staged raw scores on the fit's own masks; stage 0's
    # improvement starts from the initial prediction's loss on stage 0's out-of-bag rows
    masks = out.info["masks"]
    assert masks.shape == (8, N) and (masks.sum(1) == N // 2).all()
    raws = list(pr.staged_decision_function(X))
    init = np.tile(np.asarray(out.model["init"], dtype=np.float64), (N, 1))
    for s in range(8):
        m = masks[s].astype(bool)
        assert pr.train_score_[s] == pytest.approx(_mean_loss(name, None, raws[s][m], y[m]), rel=1e-12)
        assert oob[s] == pytest.approx(_mean_loss(name, None, raws[s][~m], y[~m]), rel=1e-12)
    m0 = masks[0].astype(bool)
    assert imp[0] == pytest.approx(_mean_loss(name, None, init[~m0], y[~m0]) - oob[0], rel=1e-9)


def test_full_sample_fit_has_no_out_of_bag_attributes():
    pr = _pair(0)[0]
    for attr in ("oob_scores_", "oob_improvement_", "oob_score_"):
        with pytest.raises(AttributeError, match="subsample < 1"):
            getattr(pr, attr)
    old = {k: v for k, v in pr.model.items() if k not in ("feature_importances", "train_score")}
    for attr in ("feature_importances_", "train_score_"):              # an artefact saved before this change
        with pytest.raises(AttributeError):
            getattr(Predictor(old), attr)


def test_early_stopped_fit_has_n_estimators_entries():
    X, y = _binned(2)
    roles = np.ones((1, N), np.uint8)
    roles[0, ::5] = 2
    out = _fit(CLS, X, y, {"n_estimators": 200, "n_iter_no_change": 2, "learning_rate": 0.5, "random_state": 0},
               staged={"scoring": "accuracy"}, split_roles=roles)
    pr = Predictor(out.model)
    S = pr.n_estimators_
    assert 2 < S < 200 and pr.train_score_.shape == (S,)
    assert len(out.info["staged"]["score"]) == len(out.info["staged"]["loss"]) == S
    # validation rows are in no category: the train curve is the loss over the other training rows
    raws = list(pr.staged_decision_function(X))
    assert len(raws) == S
    acc = [np.mean((r[roles[0] == 2, 0] >= 0) == y[roles[0] == 2]) for r in raws]
    assert out.info["staged"]["score"] == acc
    assert pr.train_score_[-1] < _mean_loss(CLS, None, raws[-1][roles[0] == 1], y[roles[0] == 1])


# ---- end to end through the client ------------------------------------------------------------
@pytest.fixture
def ctl(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), journal=str(tmp_path / "journal.jsonl"), device="cpu",
                          sse_interval_s=0.05))
    yield c
    c.shutdown()


def _client(ctl, tmp_path, is_cls):
    import pandas as pd
    from distributed_ml import MLTaskManager

    X, y = _binned(2 if is_cls else 0)
    X, y = X[:240], y[:240]
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D)])
    df["target"] = y
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    m = MLTaskManager(controller=ctl)
    assert "error" not in m.download_data(path, "toy", "local")
    return m


def _train(m, est, option, **extra):
    tp = {"target_column": "target", **extra}
    if option is not None:
        tp["staged_scores"] = option
    return m.train(est, "toy", tp, wait_for_completion=True, polling_interval=0.02)


@pytest.mark.parametrize("is_cls", [True, False])
def test_job_staged_scores(ctl, tmp_path, is_cls):
    m = _client(ctl, tmp_path, is_cls)
    GB = GradientBoostingClassifier if is_cls else GradientBoostingRegressor
    S = 6
    out = _train(m, GridSearchCV(GB(n_estimators=S, random_state=4), {"max_depth": [2, 3]}, cv=3), True)
    assert out["job_status"] == "completed", out
    for r in out["job_result"]["results"]:
        e = r["staged_scores"]
        assert e["scoring"] == ("accuracy" if is_cls else "r2") and e["n_stages"] == S
        sc = np.asarray(e["cv_scores"])
        assert sc.shape == (3, S) and len(e["mean_cv_loss"]) == len(e["holdout_score"]) == len(e["holdout_loss"]) == S
        assert e["mean_cv_score"] == sc.mean(0).tolist() and e["std_cv_score"] == sc.std(0).tolist()
        # the last stage is the model the candidate was scored with
        if is_cls:
            assert e["mean_cv_score"][-1] == pytest.approx(r["mean_cv_score"], abs=1e-15)
            assert e["holdout_score"][-1] == pytest.approx(r["accuracy"], abs=1e-15)
        else:   # the reported r2 is computed from float32 predictions (tests/test_model_predictor.py)
            assert e["mean_cv_score"][-1] == pytest.approx(r["mean_cv_score"], rel=1e-5, abs=1e-5)
            assert e["holdout_score"][-1] == pytest.approx(r["r2_score"], rel=1e-5, abs=1e-5)
        assert e["best_stage"] == int(np.argmax(e["mean_cv_score"])) + 1
        assert e["best_stage_score"] == max(e["mean_cv_score"]) == e["mean_cv_score"][e["best_stage"] - 1]
        assert np.all(np.diff(e["mean_cv_loss"]) < 0)                  # six stages of a learnable target
    assert out["best_result"]["staged_scores"] in [r["staged_scores"] for r in out["job_result"]["results"]]
    # the prefix property: stage s of the curve is the score of the same job with n_estimators = s
    first = out["job_result"]["results"][0]
    assert first["parameters"]["max_depth"] == 2
    for s in (1, 2, S):
        solo = _train(m, GridSearchCV(GB(n_estimators=s, random_state=4), {"max_depth": [2]}, cv=3), None)
        ref = solo["job_result"]["results"][0]["cv_scores"]
        got = [fold[s - 1] for fold in first["staged_scores"]["cv_scores"]]
        assert got == ref if is_cls else got == pytest.approx(ref, rel=1e-5, abs=1e-5)
    # the refit artefact: kept fits always record their training curve and importances
    path = m.download_best_model(dest=str(tmp_path / "best.npz"))
    pr = Predictor(load_model(path))
    assert pr.train_score_.shape == (S,) and pr.feature_importances_.shape == (D,)
    assert "staged_test_score" not in pr.model                        # the refit has no held-out rows
    again = Predictor(load_model(save_model(pr.model, str(tmp_path / "again.npz"))))
    np.testing.assert_array_equal(again.train_score_, pr.train_score_)
    np.testing.assert_array_equal(again.feature_importances_, pr.feature_importances_)


def test_prefix_followers_get_their_own_cut(ctl, tmp_path):
    m = _client(ctl, tmp_path, True)
    out = _train(m, GridSearchCV(GradientBoostingClassifier(random_state=2, max_depth=2), {"n_estimators": [2, 5, 3]},
                                 cv=3), {"scoring": None})
    assert out["job_status"] == "completed", out
    res = {r["parameters"]["n_estimators"]: r["staged_scores"] for r in out["job_result"]["results"]}
    assert [res[k]["n_stages"] for k in (2, 3, 5)] == [2, 3, 5]
    for k in (2, 3):
        for key in ("cv_scores", "mean_cv_score", "mean_cv_loss", "holdout_score", "holdout_loss"):
            assert np.asarray(res[k][key]).T[:k].tolist() == np.asarray(res[5][key]).T[:k].tolist(), key
        assert res[k]["mean_cv_score"][-1] == pytest.approx(
            [r for r in out["job_result"]["results"] if r["parameters"]["n_estimators"] == k][0]["mean_cv_score"], abs=1e-15)


def test_holdout_artefacts_carry_their_curves(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), device="cpu", keep_models="all"))
    try:
        m = _client(c, tmp_path, True)
        out = _train(m, GridSearchCV(GradientBoostingClassifier(random_state=2, subsample=0.5), {"n_estimators": [4, 2]},
                                     cv=2), True)
        assert out["job_status"] == "completed", out
        for r in out["job_result"]["results"]:
            k = r["parameters"]["n_estimators"]
            assert "oob_score" not in r                                # a forest's result key, not this one's
            if r["parameters"] == out["best_result"]["parameters"]:   # its artefact is the refit on every row
                continue
            hold = Predictor(load_model(r["model_path"]))
            assert hold.model["staged_test_score"].tolist() == r["staged_scores"]["holdout_score"]
            assert hold.model["staged_test_loss"].tolist() == r["staged_scores"]["holdout_loss"]
            assert hold.train_score_.shape == hold.oob_scores_.shape == hold.oob_improvement_.shape == (k,)
            assert hold.oob_score_ == hold.oob_scores_[-1] and hold.feature_importances_.shape == (D,)
        assert len(out["job_result"]["results"]) == 2
    finally:
        c.shutdown()


@pytest.mark.parametrize("option,est,message", [
    ({"scorer": "accuracy"}, "gbc", "unknown key(s) ['scorer']"),
    ("yes", "gbc", "must be true or a dict of scoring"),
    ({"scoring": "f1_macro"}, "gbc", "supported: ['accuracy']"),
    ({"scoring": "accuracy"}, "gbr", "'r2', 'neg_mean_squared_error', 'neg_root_mean_squared_error'"),
    (True, "rf", "GradientBoostingClassifier and GradientBoostingRegressor, not RandomForestClassifier"),
])
def test_validation_errors(ctl, tmp_path, option, est, message):
    from sklearn.ensemble import RandomForestClassifier

    m = _client(ctl, tmp_path, est != "gbr")
    base = {"gbc": GradientBoostingClassifier(n_estimators=2), "gbr": GradientBoostingRegressor(n_estimators=2),
            "rf": RandomForestClassifier(n_estimators=2)}[est]
    out = _train(m, GridSearchCV(base, {"max_depth": [2]}, cv=2), option)
    assert out.get("status") == "error" and message in out["message"], out


def test_regressor_scorers(ctl, tmp_path):
    m = _client(ctl, tmp_path, False)
    est = GridSearchCV(GradientBoostingRegressor(n_estimators=3, random_state=0), {"max_depth": [2]}, cv=2)
    mse = _train(m, est, {"scoring": "neg_mean_squared_error"})["job_result"]["best_result"]["staged_scores"]
    rmse = _train(m, est, {"scoring": "neg_root_mean_squared_error"})["job_result"]["best_result"]["staged_scores"]
    assert mse["scoring"] == "neg_mean_squared_error" and rmse["scoring"] == "neg_root_mean_squared_error"
    np.testing.assert_allclose(rmse["cv_scores"], -np.sqrt(-np.asarray(mse["cv_scores"])), rtol=1e-15)
    # squared_error: train_score_'s convention (twice the half loss) is the mean squared error
    np.testing.assert_allclose(mse["holdout_loss"], -np.asarray(mse["holdout_score"]), rtol=1e-12)


def test_job_without_the_option_has_none_of_it(ctl, tmp_path):
    m = _client(ctl, tmp_path, True)
    out = _train(m, GridSearchCV(GradientBoostingClassifier(n_estimators=3), {"max_depth": [2]}, cv=2), None)
    assert out["job_status"] == "completed"
    assert "staged_scores" not in out["job_result"]["best_result"]
    assert all("staged_scores" not in r for r in out["job_result"]["results"])
    raw = load_model(m.download_best_model(dest=str(tmp_path / "plain.npz")))
    assert not [k for k in raw if k.startswith("staged")]
    assert raw["train_score"].shape == (3,) and raw["feature_importances"].shape == (D,)

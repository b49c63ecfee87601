"""QuadraticDiscriminantAnalysis on the CPU data path (models/discriminant.py, docs/QDA.md): a
grid search through the client against sklearn's GridSearchCV, the kept model against sklearn's
estimator, sklearn's error and warning texts, and the host twin of the kernels against numpy.

Measured deviations (printed; run with ``-s``), largest over the three shapes of SHAPES:
kept model vs sklearn float64 ``decision_function`` 3.5e-11 absolute (at (130, 33, 2), reg_param 0:
eigh of the covariance against sklearn's SVD of the centred rows), ``predict_proba`` 1.5e-13;
host twin vs numpy float64: moments 7.0e-16 relative to the largest entry, decision values
2.9e-14 absolute.  The bounds below are 10 x those.
"""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine import model_store
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, build_tasks, prepare_splits, run_candidates
from cs230_distributed_machine_learning_amd.engine.service import Controller
from cs230_distributed_machine_learning_amd.models import discriminant
from cs230_distributed_machine_learning_amd.models.base import family_of
from cs230_distributed_machine_learning_amd.ops import qda_ops

sk = pytest.importorskip("sklearn")
from sklearn.discriminant_analysis import QuadraticDiscriminantAnalysis  # noqa: E402
from sklearn.model_selection import GridSearchCV, StratifiedKFold  # noqa: E402

SHAPES = [(96, 5, 3), (200, 17, 4), (130, 33, 2)]
REGS = [0.0, 0.1, 0.5]
DEC_TOL, PROBA_TOL = 3.5e-10, 1.5e-12     # 10 x the measured worst (module docstring)
TWIN_MOM_TOL, TWIN_DEC_TOL = 7.0e-15, 2.9e-13


def table(n, d, C):
    rng = np.random.default_rng(0)
    y = rng.integers(0, C, n)
    X = rng.normal(size=(n, d)).astype(np.float32) + (0.7 * y[:, None]).astype(np.float32)
    return X, y


def min_gap(dec):
    top = np.sort(dec, 1)
    return float((top[:, -1] - top[:, -2]).min())


@pytest.fixture
def ctl(tmp_path):
    c = Controller(Config(data_root=str(tmp_path / "data"), journal=str(tmp_path / "journal.jsonl"), device="cpu",
                          sse_interval_s=0.05))
    yield c
    c.shutdown()


@pytest.mark.parametrize("n,d,C", SHAPES)
def test_grid_search_matches_sklearn(ctl, tmp_path, n, d, C):
    import pandas as pd
    from distributed_ml import MLTaskManager

    X, y = table(n, d, C)
    X64 = X.astype(np.float64)
    search = GridSearchCV(QuadraticDiscriminantAnalysis(), {"reg_param": REGS}, cv=3)
    ref = search.fit(X64, y)
    # a label can only differ from sklearn's through a tie: the reference's own top-two gap on the
    # held-out rows of every fit is far above the decision tolerance
    gap = min(min_gap(QuadraticDiscriminantAnalysis(reg_param=r).fit(X64[tr], y[tr])._decision_function(X64[te]))
              for r in REGS for tr, te in StratifiedKFold(3).split(X64, y))
    print(f"sklearn's smallest top-two gap at {(n, d, C)}: {gap:.3e}")
    assert gap > 1000 * DEC_TOL
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(d)])
    df["target"] = y
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    m = MLTaskManager(controller=ctl)
    assert "error" not in m.download_data(path, "toy", "local")
    out = m.train(GridSearchCV(QuadraticDiscriminantAnalysis(), {"reg_param": REGS}, cv=3), "toy",
                  {"target_column": "target"}, wait_for_completion=True, polling_interval=0.02)
    assert out["job_status"] == "completed", out
    ours = {r["parameters"]["reg_param"]: r for r in out["job_result"]["results"]}
    for i, p in enumerate(ref.cv_results_["params"]):
        folds = [ref.cv_results_[f"split{k}_test_score"][i] for k in range(3)]
        assert ours[p["reg_param"]]["cv_scores"] == folds, (p, ours[p["reg_param"]]["cv_scores"], folds)
    assert out["job_result"]["best_result"]["parameters"]["reg_param"] == ref.best_params_["reg_param"]
    est = m.download_best_model(dest=str(tmp_path / "best.npz"), load=True)
    skm = ref.best_estimator_
    assert est.means_.shape == (C, d) and len(est.rotations_) == C and est.scalings_[0].shape == (d,)
    np.testing.assert_allclose(est.priors_, skm.priors_, rtol=0, atol=1e-15)
    assert (est.predict(X) == skm.predict(X64)).all() and est.score(X, y) == skm.score(X64, y)


def _family_fits(dd, params, **kw):
    spec = JobSpec("QuadraticDiscriminantAnalysis", params, cv=3, keep_models="all", **kw)
    prepare_splits(dd, spec)
    tasks, errors = build_tasks(dd, spec, range(len(params)))
    assert not errors, errors
    return tasks, family_of("QuadraticDiscriminantAnalysis").run(dd, tasks, keep_models=True)


@pytest.mark.parametrize("n,d,C", SHAPES)
def test_kept_model_matches_sklearn_on_held_out_rows(tmp_path, n, d, C):
    X, y = table(n, d, C)
    X64 = X.astype(np.float64)
    dd = DeviceData(X, y, True, "cpu")
    tasks, outs = _family_fits(dd, [{"reg_param": r} for r in REGS], holdout=False)
    worst_dec = worst_p = 0.0
    for t, o in zip(tasks, outs):
        tr, te = dd.train_rows[t.split].long().numpy(), dd.test_rows[t.split].long().numpy()
        skm = QuadraticDiscriminantAnalysis(reg_param=t.params["reg_param"]).fit(X64[tr], y[tr])
        est = model_store.Predictor(model_store.load_model(model_store.save_model(o.model, str(tmp_path / "m.npz"))))
        worst_dec = max(worst_dec, float(np.abs(est.decision_function(X[te]) - skm.decision_function(X64[te])).max()))
        worst_p = max(worst_p, float(np.abs(est.predict_proba(X[te]) - skm.predict_proba(X64[te])).max()))
        assert (o.pred.numpy() == skm.predict(X64[te])).all()
    print(f"kept model vs sklearn at {(n, d, C)}: decision {worst_dec:.3e}, proba {worst_p:.3e}")
    assert worst_dec <= DEC_TOL and worst_p <= PROBA_TOL


def test_one_sample_class_and_rank_deficient_class():
    X, y = table(96, 5, 3)
    y = np.where(np.arange(96) < 2, 3, y)             # class 3: rows 0 and 1; every fold trains on one of them
    dd = DeviceData(X, y, True, "cpu")
    spec = JobSpec("QuadraticDiscriminantAnalysis", [{}], cv=2, holdout=False)
    prepare_splits(dd, spec)
    tasks, _ = build_tasks(dd, spec, [0])
    outs = family_of("QuadraticDiscriminantAnalysis").run(dd, tasks)
    assert all(o.error == "y has only 1 sample in class 3, covariance is ill defined." for o in outs)
    X, y = table(96, 5, 3)
    X[y == 1, 4] = X[y == 1, 0]                       # class 1: two equal columns
    dd = DeviceData(X, y, True, "cpu")
    r = run_candidates(dd, JobSpec("QuadraticDiscriminantAnalysis", [{"bogus": 1}, {"reg_param": 0.5}], cv=3,
                                   holdout=False), [0, 1])
    assert r[0].ok and discriminant.NOT_FULL_RANK.format(1) in r[0].result["warnings"]
    assert "ignored unknown parameters ['bogus']" in r[0].result["warnings"]
    assert r[1].ok and "warnings" not in r[1].result


@pytest.mark.parametrize("params", [{"reg_param": 1.5}, {"reg_param": "x"}, {"tol": -1.0}, {"priors": [0.5, 0.5]},
                                    {"priors": 3}, {"store_covariance": "maybe"}])
def test_bad_parameters_raise_param_error(params):
    with pytest.raises(discriminant.ParamError):
        family_of("QuadraticDiscriminantAnalysis").resolve("QuadraticDiscriminantAnalysis", params, 100, 5, 3)


@pytest.mark.parametrize("n,d,C", SHAPES)
def test_host_twin_matches_numpy(n, d, C):
    X, y = table(n, d, C)
    X64 = X.astype(np.float64)
    shift = X64.mean(0)
    perm = np.argsort(y, kind="stable").astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(y, minlength=C))])
    M = qda_ops.class_moments(torch.from_numpy(X), torch.from_numpy(shift), torch.from_numpy(perm),
                              torch.from_numpy(off), parts=3).numpy()
    Z = np.concatenate([X64 - shift, np.ones((n, 1))], 1)
    ref = np.stack([Z[y == c].T @ Z[y == c] for c in range(C)])
    dev_m = float(np.abs(M - ref).max() / np.abs(ref).max())
    rng = np.random.default_rng(1)
    mu = rng.normal(size=(2, C, d))
    V = np.linalg.qr(rng.normal(size=(2, C, d, d)))[0]
    inv = 1.0 / rng.uniform(0.5, 2.0, size=(2, 3, C, d))
    cst = rng.normal(size=(2, 3, C))
    rows = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 3)]).astype(np.int32)
    offs = [0, len(range(0, n, 2)), len(rows)]
    pred, dec = qda_ops.score(torch.from_numpy(X), torch.from_numpy(rows), offs, *map(torch.from_numpy, (mu, V, inv, cst)),
                              want_dec=True)
    want = np.concatenate([cst[s][:, None, :] - 0.5 * np.einsum(
        "rcj,kcj->krc", np.einsum("rck,ckj->rcj", X64[rows[offs[s]:offs[s + 1]], None, :] - mu[s], V[s]) ** 2, inv[s])
        for s in range(2)], 1)
    dev_d = float(np.abs(dec.numpy() - want).max())
    print(f"twin vs numpy at {(n, d, C)}: moments {dev_m:.3e} (relative), decision {dev_d:.3e}")
    assert dev_m <= TWIN_MOM_TOL and dev_d <= TWIN_DEC_TOL
    assert min_gap(want.reshape(-1, C)) > 1000 * TWIN_DEC_TOL and (pred.numpy() == want.argmax(-1)).all()

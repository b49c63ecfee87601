"""SVC(probability=True): Platt scaling + pairwise coupling on the host (docs/SVC_PROBABILITY.md).

Reference: the worker hands the user's ``SVC(probability=True)`` to scikit-learn
(aws-prod/worker/worker.py:40, 436-455), i.e. libsvm's sigmoid_train (Lin, Lin, Weng 2007)
on the decision values of an inner 5-fold CV and multiclass_probability (Wu, Lin, Weng 2004).
The engine runs the same two recurrences (csrc/runtime/svm_prob_cpu.cpp, svm_prob.hip) on
its own inner-CV shuffle -- libsvm's scheme, not scikit-learn's random stream.
"""
import math

import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.engine.model_store import load_predictor, save_model
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.models.svm import (PLATT_CONVERGED, PLATT_ITER_CAP,
                                                               PLATT_LINE_SEARCH_FAILED, platt_folds, platt_seed,
                                                               svm_proba_numpy)
from cs230_distributed_machine_learning_amd.search.cv import ROLE_TEST, ROLE_TRAIN
from cs230_distributed_machine_learning_amd.utils import native

sk = pytest.importorskip("sklearn")
from sklearn.datasets import make_classification  # noqa: E402
from sklearn.svm import SVC  # noqa: E402

NO_PROBA = "predict_proba is not available when probability=False"


# ---- independent float64 ports (written from the formulas of the two papers) -------------
def port_platt(dec, lab):
    dec, lab = np.asarray(dec, np.float64), np.asarray(lab, np.float64)
    L = len(dec)
    prior1 = float((lab > 0).sum())
    prior0 = L - prior1
    hi, lo = (prior1 + 1.0) / (prior1 + 2.0), 1.0 / (prior0 + 2.0)
    t = np.where(lab > 0, hi, lo)

    def objective(A, B):
        z = dec * A + B
        return float(np.sum(np.where(z >= 0, t * z + np.log1p(np.exp(-np.abs(z))),
                                     (t - 1.0) * z + np.log1p(np.exp(-np.abs(z))))))

    A, B = 0.0, math.log((prior0 + 1.0) / (prior1 + 1.0))
    f = objective(A, B)
    for it in range(100):
        z = dec * A + B
        e = np.exp(-np.abs(z))
        p = np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        q = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        h11 = 1e-12 + float(np.sum(dec * dec * p * q))
        h22 = 1e-12 + float(np.sum(p * q))
        h21 = float(np.sum(dec * p * q))
        g1, g2 = float(np.sum(dec * (t - p))), float(np.sum(t - p))
        if abs(g1) < 1e-5 and abs(g2) < 1e-5:
            return A, B, it, PLATT_CONVERGED, max(abs(g1), abs(g2))
        det = h11 * h22 - h21 * h21
        dA, dB = -(h22 * g1 - h21 * g2) / det, -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= 1e-10:
            nf = objective(A + step * dA, B + step * dB)
            if nf < f + 1e-4 * step * gd:
                A, B, f = A + step * dA, B + step * dB, nf
                break
            step /= 2.0
        else:
            return A, B, it, PLATT_LINE_SEARCH_FAILED, max(abs(g1), abs(g2))
    return A, B, 100, PLATT_ITER_CAP, float("nan")


def port_coupling(dec_row, AB, k):
    """One row: (p [k], iterations, the max_error of every convergence check)."""
    r = np.zeros((k, k))
    pi = 0
    for a in range(k):
        for b in range(a + 1, k):
            z = dec_row[pi] * AB[pi, 0] + AB[pi, 1]
            s = math.exp(-z) / (1.0 + math.exp(-z)) if z >= 0 else 1.0 / (1.0 + math.exp(z))
            r[a, b] = min(max(s, 1e-7), 1.0 - 1e-7)
            r[b, a] = 1.0 - r[a, b]
            pi += 1
    Q = np.zeros((k, k))
    for t in range(k):
        for j in range(k):
            if j != t:
                Q[t, t] += r[j, t] ** 2
                Q[t, j] = -r[j, t] * r[t, j]
    p = np.full(k, 1.0 / k)
    errs = []
    it = 0
    while it < max(100, k):
        Qp = Q @ p
        pQp = float(p @ Qp)
        errs.append(float(np.abs(Qp - pQp).max()))
        if errs[-1] < 0.005 / k:
            break
        for t in range(k):
            diff = (pQp - Qp[t]) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2.0 * Qp[t])) / (1.0 + diff) ** 2
            Qp = (Qp + diff * Q[t]) / (1.0 + diff)
            p = p / (1.0 + diff)
        it += 1
    return p, it, errs


def host_pair_proba(D, AB, k):
    D, AB = np.ascontiguousarray(D, np.float64), np.ascontiguousarray(AB, np.float64)
    m = D.shape[1]
    out, iters = np.empty((m, k)), np.zeros(m, np.int32)
    assert native.cpu_lib().dml_cpu_svm_pair_proba(native.ptr(D), native.ptr(AB), m, k, native.ptr(out),
                                                   native.ptr(iters)) == 0
    return out, iters


def host_platt(cases):
    dec = np.concatenate([c[0] for c in cases] + [np.zeros(1)])
    lab = np.concatenate([c[1] for c in cases] + [np.zeros(1)]).astype(np.float64)
    lens = np.array([len(c[0]) for c in cases], np.int64)
    ol = np.ascontiguousarray(np.stack([np.concatenate([[0], np.cumsum(lens)[:-1]]), lens], 1).astype(np.int64))
    AB, st = np.zeros((len(cases), 2)), np.zeros((len(cases), 2), np.int64)
    assert native.cpu_lib().dml_cpu_svm_platt_fit(native.ptr(dec), native.ptr(lab), native.ptr(ol), len(cases),
                                                  native.ptr(AB), native.ptr(st)) == 0
    return AB, st


def platt_cases():
    """22 machines: three kinds x seven lengths, and an empty one."""
    cases = []
    for kind in ("overlap", "separable", "one class"):
        for L in (1, 2, 63, 64, 65, 257, 1000):
            rng = np.random.RandomState(100 + L)
            lab = np.where(rng.rand(L) < 0.4, 1, -1)
            if kind == "one class":
                lab = np.ones(L, dtype=lab.dtype)
            dec = lab * (0.5 + rng.rand(L)) if kind == "separable" else lab + 1.5 * rng.randn(L)
            cases.append((dec.astype(np.float64), lab.astype(np.float64)))
    cases.append((np.zeros(0), np.zeros(0)))
    return cases


def _cls_data(n, d, k, seed=0):
    X, y = make_classification(n, d, n_informative=min(d, 3), n_redundant=0, n_classes=k, n_clusters_per_class=1,
                               random_state=seed)
    return X.astype(np.float32), y


# ---- 1. coupling ------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(150, 4, 3), (300, 5, 5), (200, 3, 2)])
def test_coupling_equals_sklearn(n, d, k):
    X, y = _cls_data(n, d, k)
    est = SVC(probability=True, decision_function_shape="ovo", random_state=0).fit(X, y)
    D = est.decision_function(X)
    D = -D[None, :] if k == 2 else D.T      # binary: sklearn's sign -> positive towards classes_[0]
    AB = np.stack([est.probA_, est.probB_], 1)
    out, iters = host_pair_proba(D, AB, k)
    ref = est.predict_proba(X)
    print(f"k={k}: max |host - sklearn| = {np.abs(out - ref).max():.3e}, iterations {iters.min()}..{iters.max()}")
    assert np.abs(out - ref).max() <= 1e-10
    np.testing.assert_allclose(out.sum(1), 1.0, atol=1e-12)
    # The port takes the same iterations.  Over hundreds of rows the final max_error spreads
    # over (0, eps), so some row always ends within a factor 2 of eps = 0.005 / k (measured:
    # up to 0.98 eps for k = 3, docs/SVC_PROBABILITY.md); what makes the count no coin toss is
    # that no convergence check sits within rounding distance of eps: the port and the host
    # routine differ by ~1e-16 relative, the closest check is asserted 1e-9 relative away.
    eps = 0.005 / k
    worst, closest = 0.0, np.inf
    for i in range(n):
        p, it, errs = port_coupling(np.ascontiguousarray(D[:, i]), AB, k)
        assert it == iters[i], (i, it, iters[i])
        assert np.abs(p - out[i]).max() <= 1e-10
        worst = max(worst, errs[-1] / eps)
        closest = min(closest, min(abs(e / eps - 1.0) for e in errs))
    print(f"k={k}: largest final max_error / eps = {worst:.3f}; closest check to eps: {closest:.2e} relative")
    assert closest > 1e-9


# ---- 2. sigmoid fit -----------------------------------------------------------------------
def test_platt_fit_equals_port():
    cases = platt_cases()
    assert len(cases) == 22
    AB, st = host_platt(cases)
    for q, (dec, lab) in enumerate(cases):
        A, B, it, status, grad = port_platt(dec, lab)
        print(f"machine {q:2d} L={len(dec):4d}: A={AB[q, 0]:+.12f} B={AB[q, 1]:+.12f} iters={st[q, 0]} "
              f"status={st[q, 1]} |dA|={abs(A - AB[q, 0]):.1e} |dB|={abs(B - AB[q, 1]):.1e} grad={grad:.1e}")
        assert (it, status) == (st[q, 0], st[q, 1]), q
        assert abs(A - AB[q, 0]) <= 1e-9 and abs(B - AB[q, 1]) <= 1e-9, q
        assert status == PLATT_CONVERGED
    assert tuple(AB[-1]) == (0.0, 0.0) and tuple(st[-1]) == (0, PLATT_CONVERGED)    # L = 0


# ---- 3. the pipeline against a composed scikit-learn oracle -------------------------------
def _full_fit(X, y, params, **task_kw):
    dd = DeviceData(X, y, True, "cpu")
    dd.set_splits(np.full((1, len(y)), ROLE_TRAIN, np.uint8), ["full"])
    fam = family_of("SVC")
    rp = fam.resolve("SVC", params, len(y), X.shape[1], len(np.unique(y)))
    return fam.run(dd, [FitTask(0, 0, 0, "SVC", rp, **task_kw)], keep_models=True)[0]


def _engine_decision(Xp, yp, train, test, gamma):
    """The engine's own decision values (positive -> class 0 of the pair) of a fit on
    ``train``, for the rows of ``test`` in ascending order."""
    dd = DeviceData(Xp, yp, True, "cpu")
    roles = np.zeros((1, len(yp)), np.uint8)
    roles[0, train], roles[0, test] = ROLE_TRAIN, ROLE_TEST
    dd.set_splits(roles, ["fold"])
    fam = family_of("SVC")
    rp = fam.resolve("SVC", {"C": 1.0, "gamma": gamma}, len(train), Xp.shape[1], 2)
    return -fam.run(dd, [FitTask(0, 0, 0, "SVC", rp)])[0].decision.numpy()


@pytest.mark.parametrize("n,k", [(240, 2), (210, 3)])
def test_pipeline_matches_composed_sklearn_oracle(n, k):
    X, y = _cls_data(n, 4, k, seed=1)
    out = _full_fit(X, y, {"C": 1.0, "kernel": "rbf", "probability": True, "random_state": 0})
    model = out.model
    assert model["probability"] is True and len(model["machines"]) == k * (k - 1) // 2
    gamma = 1.0 / (X.shape[1] * X.astype(np.float64).var())    # 'scale' on the whole training split
    assert model["gamma"] == pytest.approx(gamma, rel=1e-12)
    pi, ddiff, worst, worst_own = 0, 0.0, 0.0, 0.0
    for a in range(k):
        for b in range(a + 1, k):
            rows = np.nonzero((y == a) | (y == b))[0]
            Xp, yp = X[rows], (y[rows] == b).astype(int)          # pair class a -> 0, b -> 1
            dec, own = np.zeros(len(rows)), np.zeros(len(rows))
            for ho in platt_folds(len(rows), platt_seed(0, pi)):
                rest = np.setdiff1d(np.arange(len(rows)), ho)
                ref = SVC(C=1.0, kernel="rbf", gamma=gamma).fit(Xp[rest], yp[rest])
                dec[ho] = -ref.decision_function(Xp[ho])         # internal sign: positive -> class a
                own[np.sort(ho)] = _engine_decision(Xp, yp, rest, ho, gamma)
            ddiff = max(ddiff, np.abs(own - dec).max())
            lab = np.where(yp == 0, 1.0, -1.0)
            A, B, _it, status, _g = port_platt(dec, lab)
            assert status == PLATT_CONVERGED
            m = model["machines"][pi]
            assert tuple(m["pair"]) == (a, b)
            worst = max(worst, abs(m["probA"] - A), abs(m["probB"] - B))
            A, B = port_platt(own, lab)[:2]        # the same folds solved one by one by the engine
            worst_own = max(worst_own, abs(m["probA"] - A), abs(m["probB"] - B))
            pi += 1
    # 1e-6 holds for decision values equal to 1e-9; the engine's differ from libsvm's by more
    # (float32 kernel values in the SMO, both solvers stop at tol = 1e-3), so the bound widens
    # in proportion to the difference measured here (docs/SVC_PROBABILITY.md has both numbers)
    bound = 1e-6 * max(1.0, ddiff / 1e-9)
    print(f"k={k}: engine vs sklearn held-out decision values {ddiff:.3e}; |dA|, |dB| <= {worst:.3e} "
          f"(bound {bound:.3e}); on the engine's own fold-by-fold values {worst_own:.3e}")
    assert worst <= bound
    assert worst_own <= 1e-6     # folds, row order, labels and sigmoid fit of the batched path


def test_one_class_inner_folds_take_libsvms_constants():
    """A four-fifths subset that lost class b has nothing to solve: its held-out rows get +1
    (libsvm svm_binary_svc_probability); the other folds are solved as usual."""
    rng = np.random.RandomState(3)
    X = rng.randn(15, 3).astype(np.float32)
    y = np.array([0] * 14 + [1])
    X[y == 1] += 1.5
    out = _full_fit(X, y, {"C": 1.0, "probability": True, "random_state": 0})
    m = out.model["machines"][0]
    gamma = out.model["gamma"]
    lab = np.where(y == 0, 1.0, -1.0)
    own, constants = np.zeros(len(y)), 0
    for ho in platt_folds(len(y), platt_seed(0, 0)):
        rest = np.setdiff1d(np.arange(len(y)), ho)
        if len(np.unique(y[rest])) == 1:
            own[ho] = 1.0 if y[rest][0] == 0 else -1.0
            constants += 1
        else:
            own[np.sort(ho)] = _engine_decision(X, y, rest, ho, gamma)
    assert constants == 1     # the fold that holds the only row of class 1
    A, B = port_platt(own, lab)[:2]
    assert abs(m["probA"] - A) <= 1e-6 and abs(m["probB"] - B) <= 1e-6
    proba = svm_proba_numpy(out.model, X)
    assert np.isfinite(proba).all() and np.abs(proba.sum(1) - 1.0).max() <= 1e-12


def test_coupling_beyond_one_wave_of_classes():
    """k = 70 > 64: the GPU path hands these to the host routine, which has no class limit."""
    k, m = 70, 3
    rng = np.random.RandomState(k)
    npairs = k * (k - 1) // 2
    D = 2.0 * rng.randn(npairs, m)
    AB = np.stack([rng.uniform(-3.0, -0.5, npairs), rng.uniform(-0.5, 0.5, npairs)], 1)
    out, iters = host_pair_proba(D, AB, k)
    for i in range(m):
        p, it, _errs = port_coupling(np.ascontiguousarray(D[:, i]), AB, k)
        assert it == iters[i]
        assert np.abs(p - out[i]).max() <= 1e-10
    assert np.abs(out.sum(1) - 1.0).max() <= 1e-12


# ---- 4. end to end against scikit-learn's own probabilities --------------------------------
def test_probabilities_within_sklearn_seed_spread():
    X, y = _cls_data(600, 5, 2)
    ref = [SVC(probability=True, random_state=s).fit(X, y).predict_proba(X) for s in range(5)]
    spread = max(np.abs(ref[0] - r).max() for r in ref[1:])
    out = _full_fit(X, y, {"probability": True, "random_state": 0})
    ours = svm_proba_numpy(out.model, X)
    dist = np.abs(ours - ref[0]).max()
    print(f"sklearn seed-to-seed spread {spread:.4f}; engine vs random_state=0 {dist:.4f}")
    assert dist <= 2 * spread


def test_job_ranks_candidates_by_log_loss_like_sklearn():
    from sklearn.model_selection import cross_val_score

    X, y = _cls_data(600, 5, 2)
    Cs = (0.05, 20.0)
    grid = [{"C": c, "probability": True, "random_state": 0} for c in Cs]
    res = run_candidates(DeviceData(X, y, True, "cpu"), JobSpec("SVC", grid, cv=3, scoring="neg_log_loss"), [0, 1])
    assert all(r.ok for r in res), [r.error for r in res]
    ours = [r.result["mean_cv_score"] for r in res]
    assert all(np.isfinite(r.result["cv_scores"]).all() for r in res) and all(s < 0 for s in ours)
    for s in range(5):   # the two C values are far enough apart that sklearn's order holds for every seed
        ref = [cross_val_score(SVC(C=c, probability=True, random_state=s), X, y, cv=3, scoring="neg_log_loss").mean()
               for c in Cs]
        assert ref[0] < ref[1]
        print(f"seed {s}: sklearn {ref[0]:.4f} {ref[1]:.4f}; engine {ours[0]:.4f} {ours[1]:.4f}")
    assert ours[0] < ours[1]


# ---- 5. contracts ----------------------------------------------------------------------------
def test_probability_false_fails_a_probability_scorer_with_sklearns_message():
    X, y = _cls_data(150, 4, 3)
    grid = [{"C": 1.0}, {"C": 1.0, "probability": True, "random_state": 0}]
    res = run_candidates(DeviceData(X, y, True, "cpu"),
                         JobSpec("SVC", grid, cv=3, holdout=False, keep_models="none", scoring="neg_log_loss"), [0, 1])
    assert not res[0].ok and NO_PROBA in res[0].error and "ParamError" in res[0].error
    assert res[1].ok, res[1].error       # the candidate next to it in the batch is served


@pytest.mark.parametrize("k", [2, 3])
def test_accuracy_scored_search_pays_nothing_for_the_flag(k):
    X, y = _cls_data(240, 4, k)
    fam = family_of("SVC")
    got = {}
    for flag in (False, True):
        spec = JobSpec("SVC", [{"C": 2.0, "probability": flag, "random_state": 0}], cv=3, holdout=False,
                       keep_models="none", scoring="accuracy")
        r = run_candidates(DeviceData(X, y, True, "cpu"), spec, [0])[0]
        assert r.ok, r.error
        got[flag] = (r.result["cv_scores"], fam.last_solve_stats["problems"], r.result.get("warnings", []))
    assert got[True][0] == got[False][0]
    assert got[True][1] == got[False][1] == 3 * k * (k - 1) // 2      # no inner problems were added
    assert not any("Platt" in w for w in got[True][2])


def test_artefact_predict_proba_round_trip(tmp_path):
    X, y = _cls_data(210, 4, 3, seed=1)
    labels = np.array(["ant", "bee", "cat"])[y]
    dd = DeviceData(X, labels, True, "cpu")
    roles = np.full((1, len(y)), ROLE_TRAIN, np.uint8)
    roles[0, ::4] = ROLE_TEST
    dd.set_splits(roles, ["holdout"])
    fam = family_of("SVC")
    outs = {}
    for flag in (False, True):
        rp = fam.resolve("SVC", {"C": 1.0, "probability": flag, "random_state": 3}, int((roles == ROLE_TRAIN).sum()), 4, 3)
        outs[flag] = fam.run(dd, [FitTask(0, 0, 0, "SVC", rp, need_proba=flag)], keep_models=True)[0]
    o = outs[True]
    assert o.error is None and tuple(o.proba.shape) == (len(y[::4]), 3)
    assert fam.last_solve_stats["problems"] == 6 * 3
    est = load_predictor(save_model(o.model, str(tmp_path / "svc_proba.npz")))
    Xt = X[::4]
    proba = est.predict_proba(Xt)
    np.testing.assert_allclose(proba.sum(1), 1.0, atol=1e-12)
    assert np.abs(proba - o.proba.numpy()).max() <= 1e-9
    assert list(est.classes_) == ["ant", "bee", "cat"]
    # predict is the vote, unchanged by the flag
    plain = load_predictor(save_model(outs[False].model, str(tmp_path / "svc_plain.npz")))
    assert (est.predict(Xt) == plain.predict(Xt)).all()
    assert (o.pred.numpy() == outs[False].pred.numpy()).all()
    # an artefact saved without probabilities still raises
    with pytest.raises(AttributeError, match="predict_proba"):
        plain.predict_proba(Xt)

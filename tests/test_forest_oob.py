"""oob_score=True on kept RandomForest* models: the host out-of-bag walk
(csrc/runtime/forest_oob_cpu.cpp) against an independent numpy reference, a statistical
comparison with sklearn's oob_score_, and the plumbing from the parameter to the job result."""
import os

import numpy as np
import pytest

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.engine.model_store import (Predictor, _forest_build, load_predictor,
                                                                       save_model)
from cs230_distributed_machine_learning_amd.models.base import FitTask, ParamError, family_of
from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

sk = pytest.importorskip("sklearn")
from sklearn.datasets import make_classification, make_regression  # noqa: E402

OOB_WARNING = ("Some inputs do not have OOB scores. This probably means too few trees were used to compute "
               "any reliable OOB estimates.")
CLS, REG = "RandomForestClassifier", "RandomForestRegressor"

# ---- forest_common.h splitmix64 / hash_u32 / boot_weight in Python integers ----------------------
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def hash_u32(key, ctr):
    return splitmix64(key ^ splitmix64((ctr + 0x632BE59BD9B4E019) & M64)) >> 32


def boot_weight(spec, row):
    if not int(spec["bootstrap"]):
        return 1
    u = hash_u32(int(spec["seed"]), 0xB0075 * 0x100000000 + int(row))
    cdf = [int(v) for v in spec["pois_cdf"]]
    if int(spec["bootstrap"]) == 2:
        return 1 if u < cdf[0] else 0
    return sum(1 for c in cdf if u >= c)


def _weights(specs, rows):
    return np.array([[boot_weight(s, r) for r in rows] for s in specs], dtype=np.int64)   # [T, n_rows]


# ---- data: 1000 rows, 700 of them in the split (a role vector with holes) ----------------------
N, N_TRAIN = 1000, 700
_DATA = {}


def _roles():
    r = np.random.RandomState(0).permutation(N)
    roles = np.zeros((1, N), np.uint8)
    roles[0, r[:N_TRAIN]] = 1
    roles[0, r[N_TRAIN:N_TRAIN + 200]] = 2   # 100 rows stay unused
    return roles


def _data(C):
    """C >= 2: classification with C classes; C == 0: regression."""
    if C not in _DATA:
        if C:
            X, y = make_classification(N, 8, n_informative=6, n_redundant=0, n_classes=C, random_state=21 + C)
        else:
            X, y = make_regression(N, 8, n_informative=5, noise=10, random_state=20)
            y = y / 64.0   # |y| < 8: a float32 output is within 2.4e-7 of its float64 value (the 1e-6 bound below)
        dd = DeviceData(X.astype(np.float32), y, bool(C), "cpu")
        dd.set_splits(_roles(), ["holdout"])
        _DATA[C] = dd
    return _DATA[C]


def _run_two(dd, params):
    """The fit under test as the SECOND fit of a batch (its trees start at t0 > 0 of the pool)."""
    name = CLS if dd.classification else REG
    fam = family_of(name)
    first = fam.resolve(name, {"n_estimators": 2, "max_depth": 2, "random_state": 9}, N_TRAIN, dd.d, dd.n_classes)
    rp = fam.resolve(name, params, N_TRAIN, dd.d, dd.n_classes)
    tasks = [FitTask(0, 0, 0, name, first, seed=1), FitTask(1, 1, 0, name, rp, seed=2)]
    out = fam.run(dd, tasks, keep_models=True)
    assert out[0].model is not None and "oob_score" not in out[0].model   # the first fit asked for none
    return fam, tasks[1], out[1]


def _reference(dd, model, specs):
    """Out-of-bag averages from leaf indices (forest_ops.apply) and the Python bootstrap weights."""
    fb = _forest_build(model)
    Xb = dd.binned().numpy()
    rows = dd.train_rows[0].numpy()
    leaf = forest_ops.apply(fb, Xb)[:, rows]            # [T, n_rows]
    w = _weights(specs, rows)
    if not fb.is_reg and not model["params"].get("class_weight"):
        # the reimplemented weights are the builder's: each tree's root holds their sum
        np.testing.assert_array_equal(w.sum(1).astype(np.float64), fb.vals[:fb.n_trees].sum(1))
    oob = w == 0
    v = fb.vals[leaf]                                    # [T, n_rows, VC]
    if fb.is_reg:
        ok = oob & (v[..., 0] > 0)
        cnt = ok.sum(0)
        s = np.where(ok, v[..., 1] / np.where(v[..., 0] > 0, v[..., 0], 1.0), 0.0).sum(0)
        dec = np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0)
        y = dd.y_reg.numpy().astype(np.float64)[rows]
        score = 1.0 - ((dec.astype(np.float32).astype(np.float64) - y) ** 2).sum() / ((y - y.mean()) ** 2).sum()
    else:
        cnt = oob.sum(0)
        frac = v / v.sum(2, keepdims=True)
        s = np.where(oob[..., None], frac, 0.0).sum(0)
        dec = np.where(cnt[:, None] > 0, s / np.maximum(cnt, 1)[:, None], 0.0)
        score = float(np.mean(dec.argmax(1) == dd.y_enc[rows]))
    return dec, cnt.astype(np.int32), score, fb, Xb, rows


def _check(dd, params):
    fam, task, out = _run_two(dd, params)
    m = out.model
    specs = fam._specs([task])
    dec, cnt, score, fb, Xb, rows = _reference(dd, m, specs)
    key = "oob_prediction" if fb.is_reg else "oob_decision_function"
    assert m[key].dtype == np.float32 and m["oob_rows"].dtype == np.int32
    np.testing.assert_array_equal(m["oob_rows"], rows)
    np.testing.assert_allclose(m[key], dec, rtol=0, atol=1e-6)
    # the entry point on the extracted forest (t0 == 0) gives the batch's (t0 > 0) bits, and the counts
    res = forest_ops.oob_predict(fb, Xb, specs, 0, fb.n_trees, rows)
    np.testing.assert_array_equal(res[0], m[key])
    np.testing.assert_array_equal(res[1], cnt)
    if fb.is_reg:
        assert abs(m["oob_score"] - score) < 1e-6
    else:
        # ties between two classes' float32 sums can order differently from the float64 reference's
        margin = np.sort(dec, 1)
        safe = margin[:, -1] - margin[:, -2] > 1e-5
        np.testing.assert_array_equal(res[2][safe], dec.argmax(1)[safe])
        assert abs(m["oob_score"] - score) <= (~safe).sum() / len(rows) + 1e-12
        assert m["oob_score"] == float(np.mean(res[2] == dd.y_enc[rows]))
    none = cnt == 0
    if none.any():
        assert not np.any(m[key][none]) and OOB_WARNING in out.info["warnings"]
        if not fb.is_reg:
            assert not np.any(res[2][none])
    else:
        assert OOB_WARNING not in out.info["warnings"]
    return m, cnt


def test_boot_is_oob_agrees_with_boot_weight():
    """forest_common.h boot_is_oob (one hash, one compare) == (boot_weight == 0), for the Poisson
    bootstrap, the Bernoulli subsample (bootstrap == 2, the opposite sense) and no bootstrap."""
    lib = native.cpu_lib()
    specs = forest_ops.make_specs(3)
    specs["seed"] = [0x1234ABCD5678, 77, 5]
    specs["bootstrap"] = [1, 2, 0]
    specs["pois_cdf"][0] = native.poisson_cdf_table(0.7)
    specs["pois_cdf"][1] = 0
    specs["pois_cdf"][1][0] = int(0.6 * 2**32)
    out = np.zeros(2, np.uint32)
    for t in range(3):
        zero = 0
        for row in range(400):
            lib.dml_boot_weight_oob(native.ptr(specs[t:t + 1]), row, native.ptr(out))
            assert int(out[0]) == boot_weight(specs[t], row)
            assert bool(out[1]) == (int(out[0]) == 0)
            zero += int(out[1])
        assert (zero == 0) if t == 2 else (100 < zero < 300)


@pytest.mark.parametrize("T", [1, 3, 13])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_host_oob_matches_numpy_reference_classification(T, C):
    m, cnt = _check(_data(C), {"n_estimators": T, "oob_score": True, "random_state": 4})
    if T <= 3:
        assert (cnt == 0).any()   # 0.632^T of the rows are in every tree's bag
    assert m["oob_decision_function"].shape == (N_TRAIN, C)


@pytest.mark.parametrize("T", [3, 13])
def test_host_oob_matches_numpy_reference_regression(T):
    m, cnt = _check(_data(0), {"n_estimators": T, "oob_score": True, "random_state": 4})
    assert m["oob_prediction"].shape == (N_TRAIN,)


def test_host_oob_max_samples_and_class_weight():
    _m, cnt = _check(_data(3), {"n_estimators": 13, "oob_score": True, "max_samples": 0.5, "random_state": 1})
    assert cnt.mean() > 0.55 * 13            # Poisson(0.5) leaves a row out of 60.7 % of the trees
    _check(_data(3), {"n_estimators": 7, "oob_score": True, "class_weight": "balanced", "max_depth": 5})


def test_host_oob_depth_cap_reads_the_prefix():
    """depth_cap = k on deeper trees == the whole trees of the same fit grown to max_depth = k."""
    dd = _data(3)
    fam = family_of(CLS)
    rows = dd.train_rows[0].numpy()
    got = {}
    for depth in (8, 3):
        rp = fam.resolve(CLS, {"n_estimators": 6, "max_depth": depth, "random_state": 2}, N_TRAIN, dd.d, 3)
        specs = fam._specs([FitTask(0, 0, 0, CLS, rp)])
        fb = forest_ops.build_cpu(dd.binned().numpy(), dd.y_enc, None, dd.roles_np(), specs, 3, False)
        got[depth] = (fb, specs)
    fb, specs = got[8]
    capped = forest_ops.oob_predict(fb, dd.binned().numpy(), specs, 0, 6, rows, depth_cap=3)
    whole = forest_ops.oob_predict(got[3][0], dd.binned().numpy(), got[3][1], 0, 6, rows)
    deep = forest_ops.oob_predict(fb, dd.binned().numpy(), specs, 0, 6, rows)
    for a, b in zip(capped, whole):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(deep[0], whole[0])


# ---- sklearn sanity: bootstrap streams differ, so the comparison is statistical ----------------
def _ours_oob(X, y, is_cls, seeds):
    name = CLS if is_cls else REG
    dd = DeviceData(X, y, is_cls, "cpu")
    dd.set_splits(np.ones((1, len(y)), np.uint8), ["full"])
    fam = family_of(name)
    tasks = [FitTask(i, i, 0, name, fam.resolve(name, {"n_estimators": 100, "oob_score": True, "random_state": s},
                                                len(y), dd.d, dd.n_classes)) for i, s in enumerate(seeds)]
    return [o.model["oob_score"] for o in fam.run(dd, tasks, keep_models=True)]


def test_oob_score_tracks_sklearn_classifier():
    from sklearn.ensemble import RandomForestClassifier

    X, y = make_classification(1500, 10, n_informative=6, n_classes=3, random_state=3)
    ref = [RandomForestClassifier(100, oob_score=True, random_state=s).fit(X, y).oob_score_ for s in range(10)]
    ours = _ours_oob(X, y, True, range(3))
    print("sklearn", np.mean(ref), np.std(ref), "ours", ours)
    assert abs(np.mean(ours) - np.mean(ref)) < 0.01


def test_oob_score_tracks_sklearn_regressor():
    from sklearn.ensemble import RandomForestRegressor

    X, y = make_regression(1500, 10, n_informative=6, noise=20, random_state=4)
    ref = [RandomForestRegressor(100, oob_score=True, random_state=s).fit(X, y).oob_score_ for s in range(10)]
    ours = _ours_oob(X, y, False, range(3))
    print("sklearn", np.mean(ref), np.std(ref), "ours", ours)
    assert abs(np.mean(ours) - np.mean(ref)) < 0.01


# ---- plumbing ------------------------------------------------------------------------------
def test_resolve_oob_score():
    fam = family_of(CLS)
    assert fam.resolve(CLS, {}, 100, 4, 2)["oob_score"] is False
    assert fam.resolve(CLS, {"oob_score": True}, 100, 4, 2)["oob_score"] is True
    assert fam.resolve(REG, {"oob_score": "true", "max_samples": 0.5}, 100, 4, 1)["oob_score"] is True
    for bad in ("accuracy", 2, 0.5, None, (lambda y, p: 0.0)):
        with pytest.raises(ParamError):
            fam.resolve(CLS, {"oob_score": bad}, 100, 4, 2)
    with pytest.raises(ParamError, match="Out of bag estimation only available if bootstrap=True"):
        fam.resolve(CLS, {"oob_score": True, "bootstrap": False}, 100, 4, 2)
    fam.resolve(CLS, {"oob_score": False, "bootstrap": False}, 100, 4, 2)


def _job_data(is_cls):
    if is_cls:
        X, y = make_classification(400, 8, n_informative=5, n_classes=3, random_state=8)
        y = np.array(["ant", "bee", "cat"])[y]
    else:
        X, y = make_regression(400, 8, n_informative=5, noise=5, random_state=8)
    return X.astype(np.float32), y


@pytest.mark.parametrize("is_cls", [True, False])
def test_job_result_carries_oob_score(is_cls, monkeypatch, tmp_path):
    X, y = _job_data(is_cls)
    name = CLS if is_cls else REG
    calls = []
    real = forest_ops.oob_predict
    monkeypatch.setattr(forest_ops, "oob_predict", lambda *a, **k: (calls.append(a[3:5]), real(*a, **k))[1])
    cands = [{"n_estimators": 30, "oob_score": True, "max_depth": 6, "random_state": 0},
             {"n_estimators": 10, "oob_score": True, "bootstrap": False},
             {"n_estimators": 20, "oob_score": False},
             {"n_estimators": 20, "oob_score": True, "max_depth": 6, "random_state": 0}]   # a prefix of candidate 0
    dd = DeviceData(X, y, is_cls, "cpu")
    res = run_candidates(dd, JobSpec(name, cands, cv=2, holdout=True, keep_models="best"), range(4))
    assert len(calls) == 2                 # the two kept holdout fits with oob_score; no CV fit, no other fit
    assert not res[1].ok and "Out of bag estimation only available if bootstrap=True" in res[1].error
    hold = dd.split_names.index("holdout")
    train = dd.train_rows[hold].numpy()
    keys = ("oob_score", "oob_rows", "oob_decision_function", "oob_prediction")
    assert res[2].ok and "oob_score" not in res[2].result and not any(k in res[2].model for k in keys)
    for r in (res[0], res[3]):
        assert r.ok and r.result["oob_score"] == r.model["oob_score"]
        est = load_predictor(save_model(r.model, os.path.join(tmp_path, f"m{r.candidate}.npz")))
        assert est.oob_score_ == r.result["oob_score"]
        np.testing.assert_array_equal(est.oob_rows_, train)
        assert est.oob_rows_.dtype == np.int32
        if is_cls:
            dec = est.oob_decision_function_
            np.testing.assert_array_equal(dec, r.model["oob_decision_function"])
            assert dec.shape == (len(train), 3) and dec.dtype == np.float32
            has = dec.sum(1) > 0
            np.testing.assert_allclose(dec[has].sum(1), 1.0, atol=1e-5)
            # columns are in classes_ order: the labels of the row maxima score the stored accuracy
            acc = np.mean(est.classes_[dec.argmax(1)] == y[train])
            assert abs(acc - est.oob_score_) < 0.01
            with pytest.raises(AttributeError):
                est.oob_prediction_
        else:
            np.testing.assert_array_equal(est.oob_prediction_, r.model["oob_prediction"])
            assert est.oob_prediction_.shape == (len(train),)
            with pytest.raises(AttributeError):
                est.oob_decision_function_
        assert 0.3 < est.oob_score_ <= 1.0
        np.testing.assert_array_equal(est.feature_importances_, r.model["feature_importances"])
    # the prefix fit's out-of-bag estimate is its own (20 of the 30 trees), not the leader's
    assert res[3].model["n_trees"] == 20 and res[3].result["oob_score"] != res[0].result["oob_score"]
    # keep_models="none": nothing is computed
    calls.clear()
    res = run_candidates(dd, JobSpec(name, cands, cv=2, holdout=True, keep_models="none"), range(4))
    assert not calls and all("oob_score" not in r.result for r in res)
    assert res[0].ok and res[0].model is None


def test_cv_scores_do_not_depend_on_oob_score():
    X, y = _job_data(True)
    out = []
    for flag in (True, False):
        cands = [{"n_estimators": 15, "oob_score": flag, "random_state": 1}]
        r = run_candidates(DeviceData(X, y, True, "cpu"), JobSpec(CLS, cands, cv=3, holdout=True), [0])[0]
        out.append((r.result["cv_scores"], r.result["accuracy"]))
    assert out[0] == out[1]


def test_predictor_without_oob_raises():
    X, y = _job_data(True)
    r = run_candidates(DeviceData(X, y, True, "cpu"), JobSpec(CLS, [{"n_estimators": 5}], cv=0, holdout=True), [0])[0]
    est = Predictor(r.model)
    for attr in ("oob_score_", "oob_decision_function_", "oob_prediction_", "oob_rows_"):
        with pytest.raises(AttributeError):
            getattr(est, attr)
    assert est.feature_importances_.shape == (8,)

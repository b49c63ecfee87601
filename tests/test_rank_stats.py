"""Batched ranking and probability scorers on the CPU data path (docs/RANK_SCORES.md): the host
twin of csrc/kernels/rank_stats.hip against ``numpy.sort``, ``scoring.score`` and
``sklearn.metrics``; the errors; a multi-metric forest job that calls ``scoring.score`` for none
of its metrics; and an SVC job (float64 decision values) that stays per fit.

Cases: tests/rank_stats_cases.py (the lengths 0, 1, 2, 63, 64, 65, 257, tile - 1, tile, tile + 1,
2 * tile + 3, then a fit without a positive, one without a negative, one with one of each).

Tolerances.  roc_auc* is one division of exact integers on both routes: ``==``.  top_k_accuracy is
a count over n: ``==``.  average_precision, neg_log_loss and neg_brier_score are float64 sums of
same-signed terms added in different orders: rel 1e-12, the project's figure for such sums
(tests/test_score_stats_gpu.py); the largest differences seen here are 2.2e-16, 3.2e-16 and
4.2e-16.  sklearn is compared with ``pytest.approx`` (rel 1e-6: its log_loss renormalises float32
rows that sum to 1 within 1e-7)."""
import json

import numpy as np
import pytest
import torch

import rank_stats_cases as rc
from cs230_distributed_machine_learning_amd.config import Config
from cs230_distributed_machine_learning_amd.engine import executor
from cs230_distributed_machine_learning_amd.engine.service import Controller
from cs230_distributed_machine_learning_amd.search import scoring
from cs230_distributed_machine_learning_amd.utils import native

sk = pytest.importorskip("sklearn")
from sklearn import metrics as skm  # noqa: E402

TILE = int(native.cpu_lib().dml_cpu_rank_stats_tile())


def _same(a, b):
    return a == b or (a != a and b != b)


# ---- the sort ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rc.KEY_KINDS)
def test_segmented_sort_equals_numpy(kind):
    keys, off = rc.sort_case(TILE, kind, seed=11)
    out = scoring.segmented_sort_u32(torch.from_numpy(keys.view(np.int32)), off)
    assert out.dtype == torch.int32
    assert out.numpy().view(np.uint32).tobytes() == rc.sorted_segments(keys, off).tobytes()
    # segments that do not cover the keys: the rest is unchanged
    part = scoring.segmented_sort_u32(torch.from_numpy(keys.view(np.int32)), off[3:6]).numpy().view(np.uint32)
    ref = keys.copy()
    ref[off[3]:off[5]] = rc.sorted_segments(keys, off)[off[3]:off[5]]
    assert part.tobytes() == ref.tobytes()
    with pytest.raises(ValueError, match="seg_off"):
        scoring.segmented_sort_u32(torch.from_numpy(keys.view(np.int32)), [0, keys.size + 1])


# ---- binary problems (K = 1) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def binary_cases():
    out = {}
    for q, kind in enumerate(rc.SCORE_KINDS):
        rows, off, s, y = rc.binary_case(TILE, kind, seed=20 + q, prevalence=(0.4, 0.05, 0.5, 0.9, 0.4)[q])
        st = scoring.rank_statistics(torch.from_numpy(rows), off, torch.from_numpy(s), torch.from_numpy(y), 2,
                                     pos0=1, want=scoring.WANT_AP)
        out[kind] = (rows, off, s, y, st)
    return out


@pytest.mark.parametrize("kind", rc.SCORE_KINDS)
def test_binary_rank_scores(binary_cases, kind):
    rows, off, s, y, st = binary_cases[kind]
    F = len(off) - 1
    assert st.shape == (F, 1) and st.dtype == scoring.RANK_DTYPE
    np.testing.assert_array_equal(st["n_neg"][:, 0] + st["n_pos"][:, 0], np.diff(off))
    assert st["n_pos"][F - 3, 0] == 0 and st["n_neg"][F - 2, 0] == 0           # the one-sided fits
    assert st["n_pos"][F - 1, 0] == 1 and st["n_neg"][F - 1, 0] == 1
    worst = 0.0
    for f in range(F):
        yf = y[rows[off[f]:off[f + 1]]]
        sf = s[off[f]:off[f + 1]]
        ty, ts = torch.from_numpy(yf), torch.from_numpy(sf)
        auc = scoring.score_from_rank_stats("roc_auc", st[f], 2)
        ap = scoring.score_from_rank_stats("average_precision", st[f], 2)
        ref_auc = scoring.score("roc_auc", ty, ty, 2, None, decision=ts)
        ref_ap = scoring.score("average_precision", ty, ty, 2, None, decision=ts)
        assert _same(auc, ref_auc), (kind, f, auc, ref_auc)
        if ref_ap != ref_ap or ap != ap:
            assert _same(ap, ref_ap), (kind, f, ap, ref_ap)
        else:
            worst = max(worst, abs(ap - ref_ap) / abs(ref_ap))
            assert ap == pytest.approx(ref_ap, rel=1e-12, abs=0)
        if kind != "inf" and 0 < yf.sum() < yf.size:   # sklearn refuses inf and one-class targets
            assert auc == pytest.approx(skm.roc_auc_score(yf, sf.astype(np.float64)))
            assert ap == pytest.approx(skm.average_precision_score(yf, sf.astype(np.float64)))
    print(kind, "average_precision: largest relative difference to scoring.score", worst)


def test_zero_signs_are_one_score():
    """-0.0 and +0.0 compare equal: a positive at -0.0 and a negative at +0.0 are a tie."""
    y = torch.tensor([1, 0, 1, 0], dtype=torch.int32)
    s = torch.tensor([-0.0, 0.0, 0.0, -0.0], dtype=torch.float32)
    rows = torch.arange(4, dtype=torch.int32)
    st = scoring.rank_statistics(rows, [0, 4], s, y, 2, want=scoring.WANT_AP)
    assert int(st["u2"][0, 0]) == 4 and scoring.score_from_rank_stats("roc_auc", st[0], 2) == 0.5
    assert scoring.score_from_rank_stats("average_precision", st[0], 2) == 0.5


# ---- K = C problems and the probability sums -----------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 5, 64])
@pytest.mark.parametrize("kind", ["grid", "continuous"])
def test_multiclass_rank_and_probability_scores(C, kind):
    rows, off, p, y = rc.proba_case(TILE, C, kind, seed=30 + C)
    tr, tp, ty = torch.from_numpy(rows), torch.from_numpy(p), torch.from_numpy(y)
    st = scoring.rank_statistics(tr, off, tp, ty, C, pos0=0)
    ps = scoring.proba_statistics(tr, off, tp, ty, C, want=scoring.proba_want(scoring.PROBA_SUM_SCORERS))
    F = len(off) - 1
    assert st.shape == (F, C) and ps.shape == (F,)
    np.testing.assert_array_equal(ps["n"], np.diff(off))
    np.testing.assert_array_equal((st["n_neg"] + st["n_pos"])[:, 0], np.diff(off))
    worst = {}
    for f in range(F):
        yf = y[rows[off[f]:off[f + 1]]]
        pf = p[off[f]:off[f + 1]]
        tyf, tpf = torch.from_numpy(yf), torch.from_numpy(pf)
        for name in ("roc_auc_ovr", "roc_auc_ovr_weighted"):
            v = scoring.score_from_rank_stats(name, st[f], C)
            assert _same(v, scoring.score(name, tyf, tyf, C, tpf)), (name, f)
            if len(np.unique(yf)) == C and C > 2 and kind == "continuous":
                p64 = pf.astype(np.float64)
                sk_v = skm.roc_auc_score(yf, p64 / p64.sum(1, keepdims=True), multi_class="ovr",
                                         average="weighted" if name.endswith("weighted") else "macro")
                assert v == pytest.approx(sk_v)
        if C == 2:
            b = scoring.score_from_rank_stats("roc_auc", st[f], 2)   # the last column is the positive class
            assert _same(b, scoring.score("roc_auc", tyf, tyf, 2, tpf))
        for name in scoring.PROBA_SUM_SCORERS:
            v = scoring.score_from_rank_stats(name, ps[f], C)
            ref = scoring.score(name, tyf, tyf, C, tpf)
            if name == "top_k_accuracy" or ref != ref or ref == 0.0:
                assert _same(v, ref), (name, f, v, ref)
            else:
                worst[name] = max(worst.get(name, 0.0), abs(v - ref) / abs(ref))
                assert v == pytest.approx(ref, rel=1e-12, abs=0), (name, f)
        if yf.size:
            p64 = pf.astype(np.float64)
            onehot = np.eye(C)[yf]
            brier = ((p64[:, 1] - yf) ** 2).mean() if C == 2 else ((p64 - onehot) ** 2).sum(1).mean()
            assert scoring.score_from_rank_stats("neg_brier_score", ps[f], C) == pytest.approx(-brier)
            assert scoring.score_from_rank_stats("neg_log_loss", ps[f], C) == pytest.approx(
                -skm.log_loss(yf, p64, labels=list(range(C))))
            if C > 2:
                hits = sum((pf[i] > pf[i, t]).sum() + (pf[i, t + 1:] == pf[i, t]).sum() < 2 for i, t in enumerate(yf))
                assert scoring.score_from_rank_stats("top_k_accuracy", ps[f], C) == hits / yf.size
    print(C, kind, "largest relative differences to scoring.score", worst)


# ---- errors --------------------------------------------------------------------------------------
def test_bad_entries_raise_and_name_the_fit():
    rows, off, s, y = rc.binary_case(TILE, "continuous", seed=4)
    tr, ts, ty = torch.from_numpy(rows), torch.from_numpy(s), torch.from_numpy(y)
    bad_s = s.copy()
    bad_s[off[5] + 3] = np.nan
    with pytest.raises(ValueError, match=r"rank_statistics: fit 5 has 1 "):
        scoring.rank_statistics(tr, off, torch.from_numpy(bad_s), ty, 2)
    bad_r = rows.copy()
    bad_r[off[7] + 1] = rc.N_Y
    bad_r[off[11] - 1] = -3   # the last entry of the three-tile fit
    with pytest.raises(ValueError, match=r"rank_statistics: fit 7 has 1 "):
        scoring.rank_statistics(torch.from_numpy(bad_r), off, ts, ty, 2)
    p = np.stack([1 - np.clip(s, 0, 1), np.clip(s, 0, 1)], 1).astype(np.float32)
    with pytest.raises(ValueError, match=r"proba_statistics: fit 7 has 1 "):
        scoring.proba_statistics(torch.from_numpy(bad_r), off, torch.from_numpy(p), ty, 2, want=7)
    p[off[4], 0] = np.nan
    with pytest.raises(ValueError, match=r"proba_statistics: fit 4 has 1 "):
        scoring.proba_statistics(tr, off, torch.from_numpy(p), ty, 2, want=7)
    with pytest.raises(ValueError, match="float32"):
        scoring.rank_statistics(tr, off, ts.double(), ty, 2)
    with pytest.raises(ValueError, match="fit_row_off"):
        scoring.rank_statistics(tr, off[:-1], ts, ty, 2)
    with pytest.raises(ValueError, match="not computable"):
        scoring.score_from_rank_stats("roc_auc_ovo", None, 3)


# ---- the executor --------------------------------------------------------------------------------
N, D = 300, 6
METRICS = ["accuracy", "roc_auc", "average_precision", "neg_log_loss"]


@pytest.fixture
def client(tmp_path):
    import pandas as pd
    from distributed_ml import MLTaskManager

    rng = np.random.RandomState(5)
    X = rng.normal(size=(N, D)).astype(np.float32)
    z = 2.0 * X[:, 0] - X[:, 1] + 1.5 * rng.normal(size=N)   # noisy: probabilities strictly between the classes
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D)])
    df["target"] = (z > np.median(z)).astype(np.int64)
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    c = Controller(Config(data_root=str(tmp_path / "data"), device="cpu", sse_interval_s=0.05))
    m = MLTaskManager(controller=c)
    assert "error" not in m.download_data(path, "toy", "local")
    yield m
    c.shutdown()


def _train(m, est, **extra):
    out = m.train(est, "toy", {"target_column": "target", **extra}, wait_for_completion=True, polling_interval=0.02)
    assert out["job_status"] == "completed", out
    return {json.dumps(r["parameters"], sort_keys=True): r for r in out["job_result"]["results"]}


def _count_scores(monkeypatch):
    calls, real = [], scoring.score

    def counted(name, *a, **k):
        calls.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(scoring, "score", counted)
    return calls


def test_multimetric_forest_job_scores_nothing_per_fit(client, monkeypatch):
    """Without a holdout split (whose legacy ``accuracy`` key is a per-fit call by design) the job
    calls ``scoring.score`` for none of its four metrics; with the default holdout it does not for
    the three ranking / probability metrics, and the scores equal the per-fit route's."""
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import GridSearchCV

    est = GridSearchCV(RandomForestClassifier(n_estimators=7, random_state=0), {"max_depth": [2, None]}, cv=3,
                       scoring=METRICS, refit="roc_auc")
    calls = _count_scores(monkeypatch)
    no_hold = _train(client, est, holdout=False)
    assert [c for c in calls if c in METRICS] == [], calls
    assert all(len(r["scores"]["roc_auc"]["cv_scores"]) == 3 for r in no_hold.values())
    del calls[:]
    batched = _train(client, est)
    assert [c for c in calls if c != "accuracy"] == [] and len(calls) == 2, calls   # the two holdout fits' legacy key
    monkeypatch.setattr(executor, "_rank_proba_scores", lambda *a, **k: {})
    del calls[:]
    per_fit = _train(client, est)
    assert sum(c == "roc_auc" for c in calls) == 2 * 4   # 2 candidates x (3 folds + the holdout)
    worst = 0.0
    for key, r in batched.items():
        assert r["scoring"] == "roc_auc"
        for name in METRICS:
            e, ref = r["scores"][name], per_fit[key]["scores"][name]
            got = e["cv_scores"] + [e["holdout_score"]]
            want = ref["cv_scores"] + [ref["holdout_score"]]
            if name in ("accuracy", "roc_auc"):
                assert got == want, name
            else:
                worst = max(worst, max(abs(a - b) / abs(b) for a, b in zip(got, want)))
                assert got == pytest.approx(want, rel=1e-12, abs=0), name
        assert 0.6 < r["scores"]["roc_auc"]["mean_cv_score"] < 1.0
        assert r["cv_scores"] == r["scores"]["roc_auc"]["cv_scores"]
    print("largest relative difference, batched against per-fit", worst)


def test_float64_scores_stay_per_fit(client, monkeypatch):
    """SVC hands over float64 decision values: nothing is batched, and every roc_auc in the result
    is what ``scoring._auc`` gives for that fit's float64 values."""
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC

    ranked, seen = [], []
    real_rank, real_score = scoring.rank_statistics, scoring.score

    def score(name, y, pred, n_classes=2, proba=None, decision=None):
        v = real_score(name, y, pred, n_classes, proba, decision=decision)
        if name == "roc_auc":
            src = proba[:, 1] if proba is not None else decision
            assert src.dtype == torch.float64
            assert v == scoring._auc(y, src)
            seen.append(v)
        return v

    monkeypatch.setattr(scoring, "rank_statistics", lambda *a, **k: ranked.append(1) or real_rank(*a, **k))
    monkeypatch.setattr(scoring, "score", score)
    res = _train(client, GridSearchCV(SVC(), {"C": [0.5, 2.0]}, cv=3, scoring=["roc_auc", "accuracy"], refit="roc_auc"))
    assert ranked == [] and len(seen) == 2 * 4
    for r in res.values():
        e = r["scores"]["roc_auc"]
        assert all(v in seen for v in e["cv_scores"] + [e["holdout_score"]])
        assert 0.5 < e["mean_cv_score"] <= 1.0

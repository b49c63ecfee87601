"""csrc/kernels/rank_stats.hip on the MI355X: the segmented radix sort against ``numpy.sort``, the
rank and probability statistics against the host twin (csrc/runtime/rank_stats_cpu.cpp) on the
cases of tests/rank_stats_cases.py, a multi-metric forest job on the GPU data path against the
same job on the CPU data path, and a single-metric roc_auc job against per-fit ``scoring.score``
(docs/RANK_SCORES.md).

Tolerances: the sorted keys, n_neg, n_pos, U2, the top-2 hits, n and the bad counts are integers,
compared bit for bit.  The average precision and the Brier sum are float64 sums whose terms and
order of addition are the same on both sides, the sum of logarithms has the device's log against
the host's: all three at rtol = 1e-12 (same-signed terms, so a sum's relative error is at most its
terms'), the figures printed before they are asserted.  On an MI355X the average precision and
the Brier sum came out bit-equal on every case, the sum of logarithms on 7 of 8 (C = 2 grid:
2.0e-16 relative)."""
import json

import numpy as np
import pytest
import torch

import rank_stats_cases as rc
from cs230_distributed_machine_learning_amd.search import scoring
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu


def _tile():
    tile = int(native.hip_lib().dml_rank_stats_tile())
    assert tile == int(native.cpu_lib().dml_cpu_rank_stats_tile())
    return tile


def _dev_sort(keys, off):
    out = scoring.segmented_sort_u32(torch.from_numpy(keys.view(np.int32)).cuda(), off)
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", rc.KEY_KINDS)
def test_segmented_sort_equals_numpy(kind):
    keys, off = rc.sort_case(_tile(), kind, seed=11)   # every length in one launch
    assert _dev_sort(keys, off).tobytes() == rc.sorted_segments(keys, off).tobytes()


def test_segmented_sort_more_segments_than_a_launch_chunk():
    """70,000 segments of 0 to 3 keys (grid.y holds 65,535), then one of a tile and a half; the keys
    before the first and after the last segment are not touched."""
    rng = np.random.RandomState(3)
    lens = np.concatenate([rng.randint(0, 4, size=70000), [_tile() + _tile() // 2]])
    off = (7 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    keys = rng.randint(0, 2 ** 32, size=int(off[-1]) + 5, dtype=np.uint64).astype(np.uint32)
    out = _dev_sort(keys, off)
    assert out.tobytes() == rc.sorted_segments(keys, off).tobytes()
    assert (out[:7] == keys[:7]).all() and (out[-5:] == keys[-5:]).all()


def _rel(dev, host):
    return float(np.max(np.abs(dev - host) / np.maximum(np.abs(host), 1e-300))) if dev.size else 0.0


@pytest.mark.parametrize("kind", rc.SCORE_KINDS)
def test_binary_rank_statistics_equal_the_twin(kind, monkeypatch):
    rows, off, s, y = rc.binary_case(_tile(), kind, seed=40)
    host = scoring.rank_statistics(torch.from_numpy(rows), off, torch.from_numpy(s), torch.from_numpy(y), 2,
                                   want=scoring.WANT_AP)
    args = (torch.from_numpy(rows).cuda(), off, torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda(), 2)
    dev = scoring.rank_statistics(*args, want=scoring.WANT_AP)
    for name in ("n_neg", "n_pos", "u2"):
        np.testing.assert_array_equal(dev[name], host[name])
    print(kind, "average precision: largest relative difference", _rel(dev["ap"], host["ap"]),
          "bit-equal" if dev["ap"].tobytes() == host["ap"].tobytes() else "not bit-equal")
    np.testing.assert_allclose(dev["ap"], host["ap"], rtol=1e-12, atol=0)
    assert scoring.rank_statistics(*args, want=scoring.WANT_AP).tobytes() == dev.tobytes()   # the same bytes every run
    no_ap = scoring.rank_statistics(*args)
    assert not no_ap["ap"].any() and no_ap["u2"].tobytes() == dev["u2"].tobytes()
    monkeypatch.setattr(scoring, "RANK_CHUNK_KEYS", 5000)   # several chunks of fits, the long fit alone
    assert scoring.rank_statistics(*args, want=scoring.WANT_AP).tobytes() == dev.tobytes()


@pytest.mark.parametrize("C", [2, 3, 5, 64])
@pytest.mark.parametrize("kind", ["grid", "continuous"])
def test_multiclass_statistics_equal_the_twin(C, kind):
    rows, off, p, y = rc.proba_case(_tile(), C, kind, seed=50 + C)
    cpu = (torch.from_numpy(rows), off, torch.from_numpy(p), torch.from_numpy(y), C)
    gpu = (cpu[0].cuda(), off, cpu[2].cuda(), cpu[3].cuda(), C)
    host, dev = scoring.rank_statistics(*cpu, pos0=0), scoring.rank_statistics(*gpu, pos0=0)
    assert dev.shape == (len(off) - 1, C) and dev.tobytes() == host.tobytes()
    hp, dp = scoring.proba_statistics(*cpu, want=7), scoring.proba_statistics(*gpu, want=7)
    for name in ("n", "top2", "bad"):
        np.testing.assert_array_equal(dp[name], hp[name])
    for name in ("log", "brier"):
        print(C, kind, name, "largest relative difference", _rel(dp[name], hp[name]),
              "bit-equal" if dp[name].tobytes() == hp[name].tobytes() else "not bit-equal")
        np.testing.assert_allclose(dp[name], hp[name], rtol=1e-12, atol=0)
    d0 = scoring.proba_statistics(*gpu, want=scoring.WANT_TOP2)
    assert not d0["log"].any() and not d0["brier"].any() and d0["top2"].tobytes() == dp["top2"].tobytes()


def test_device_division_reproduces_score_on_device_tensors():
    """``scoring.score`` on device tensors divides by multiplying with a reciprocal; the
    single-metric GPU path asks ``score_from_rank_stats`` for the same form: the same doubles."""
    rows, off, s, y = rc.binary_case(_tile(), "continuous", seed=61)
    ty, ts = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    st = scoring.rank_statistics(torch.from_numpy(rows).cuda(), off, ts, ty, 2)
    differs = 0
    for f in range(len(off) - 1):
        yf = ty[torch.from_numpy(rows[off[f]:off[f + 1]]).cuda().long()]
        ref = scoring.score("roc_auc", yf, yf, 2, None, decision=ts[off[f]:off[f + 1]])
        got = scoring.score_from_rank_stats("roc_auc", st[f], 2, device_division=True)
        assert got == ref or (got != got and ref != ref), (f, got, ref)
        differs += got != scoring.score_from_rank_stats("roc_auc", st[f], 2) and got == got
    print("fits whose last place depends on the form of the division:", differs)
    rows, off, p, y = rc.proba_case(_tile(), 3, "continuous", seed=62)
    ty, tp = torch.from_numpy(y).cuda(), torch.from_numpy(p).cuda()
    st = scoring.rank_statistics(torch.from_numpy(rows).cuda(), off, tp, ty, 3, pos0=0)
    for f in range(len(off) - 1):
        yf = ty[torch.from_numpy(rows[off[f]:off[f + 1]]).cuda().long()]
        for name in ("roc_auc_ovr", "roc_auc_ovr_weighted"):
            ref = scoring.score(name, yf, yf, 3, tp[off[f]:off[f + 1]])
            got = scoring.score_from_rank_stats(name, st[f], 3, device_division=True)
            assert got == ref or (got != got and ref != ref), (name, f, got, ref)


def test_bad_entries_are_counted_like_the_twin():
    rows, off, s, y = rc.binary_case(_tile(), "continuous", seed=4)
    rows, s = rows.copy(), s.copy()
    s[off[5] + 3] = np.nan
    rows[off[7] + 1] = rc.N_Y          # never dereferenced
    rows[off[11] - 1] = -3             # the last entry of the three-tile fit
    rows[off[11] - 2] = 2 ** 31 - 1
    p = np.stack([1 - np.clip(s, 0, 1), np.clip(s, 0, 1)], 1).astype(np.float32)
    msgs = []
    for dev in ("cpu", "cuda"):
        t = [torch.from_numpy(a).to(dev) for a in (rows, s, y, p)]
        with pytest.raises(ValueError, match="rank_statistics: fit 5 has 1 ") as e1:
            scoring.rank_statistics(t[0], off, t[1], t[2], 2, want=1)
        with pytest.raises(ValueError, match="proba_statistics: fit 5 has 1 ") as e2:
            scoring.proba_statistics(t[0], off, t[3], t[2], 2, want=7)
        clean = torch.from_numpy(np.nan_to_num(s)).to(dev)
        with pytest.raises(ValueError, match="rank_statistics: fit 7 has 1 ") as e3:
            scoring.rank_statistics(t[0], off, clean, t[2], 2)
        msgs.append((str(e1.value), str(e2.value), str(e3.value)))
    assert msgs[0] == msgs[1]


N, D = 300, 6


def _toy(tmp_path):
    import pandas as pd

    rng = np.random.RandomState(5)
    X = rng.normal(size=(N, D)).astype(np.float32)
    z = 2.0 * X[:, 0] - X[:, 1] + 1.5 * rng.normal(size=N)
    df = pd.DataFrame(X, columns=[f"f{j}" for j in range(D)])
    df["target"] = (z > np.median(z)).astype(np.int64)
    path = str(tmp_path / "toy.csv")
    df.to_csv(path, index=False)
    return path


def _job(tmp_path, device, scoring_opt, refit=True, tag=""):
    from distributed_ml import MLTaskManager
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import GridSearchCV

    from cs230_distributed_machine_learning_amd.config import Config
    from cs230_distributed_machine_learning_amd.engine.service import Controller

    c = Controller(Config(data_root=str(tmp_path / f"data_{device}{tag}"), device=device, sse_interval_s=0.05))
    try:
        m = MLTaskManager(controller=c)
        assert "error" not in m.download_data(_toy(tmp_path), "toy", "local")
        # fully grown trees have pure leaves and 4 or 8 trees average to multiples of 1/8: the
        # probabilities are the same float32 on both data paths, whatever the order they are added in
        est = GridSearchCV(RandomForestClassifier(random_state=0), {"n_estimators": [4, 8]}, cv=3,
                           scoring=scoring_opt, refit=refit)
        out = m.train(est, "toy", {"target_column": "target"}, wait_for_completion=True, polling_interval=0.02)
        assert out["job_status"] == "completed", out
        return {json.dumps(r["parameters"], sort_keys=True): r for r in out["job_result"]["results"]}
    finally:
        c.shutdown()


def test_multimetric_job_on_the_gpu_equals_the_cpu_job(tmp_path, monkeypatch):
    metrics = ["accuracy", "roc_auc", "average_precision", "neg_log_loss"]
    calls, real = [], scoring.score
    monkeypatch.setattr(scoring, "score", lambda name, *a, **k: calls.append(name) or real(name, *a, **k))
    gpu = _job(tmp_path, "cuda", metrics, refit="roc_auc")
    assert [c for c in calls if c != "accuracy"] == [], calls
    cpu = _job(tmp_path, "cpu", metrics, refit="roc_auc")
    for key, r in gpu.items():
        for name in metrics:
            e, ref = r["scores"][name], cpu[key]["scores"][name]
            got, want = e["cv_scores"] + [e["holdout_score"]], ref["cv_scores"] + [ref["holdout_score"]]
            print(name, got, want)
            if name in ("accuracy", "roc_auc"):
                assert got == want, name
            else:
                assert got == pytest.approx(want, rel=1e-12, abs=0), name
        assert 0.6 < r["scores"]["roc_auc"]["mean_cv_score"] < 1.0


def test_single_metric_roc_auc_job_keeps_its_bits(tmp_path, monkeypatch):
    """scoring="roc_auc" on the GPU data path: the batched cv_scores are the doubles that per-fit
    ``scoring.score`` gives on the same fits (the batched path switched off)."""
    from cs230_distributed_machine_learning_amd.engine import executor

    ranked, real = [], scoring.rank_statistics
    monkeypatch.setattr(scoring, "rank_statistics", lambda *a, **k: ranked.append(1) or real(*a, **k))
    batched = _job(tmp_path, "cuda", "roc_auc", tag="_a")
    n_calls = len(ranked)
    assert n_calls >= 1                        # the job's CV fits went through the kernels
    monkeypatch.setattr(executor, "_rank_proba_scores", lambda *a, **k: {})
    per_fit = _job(tmp_path, "cuda", "roc_auc", tag="_b")
    assert len(ranked) == n_calls
    for key, r in batched.items():
        print(r["cv_scores"], per_fit[key]["cv_scores"])
        assert r["cv_scores"] == per_fit[key]["cv_scores"] and len(r["cv_scores"]) == 3
        assert r["mean_cv_score"] == per_fit[key]["mean_cv_score"]
        assert "scores" not in r

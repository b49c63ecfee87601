"""SVC(probability=True) on the MI355X: csrc/kernels/svm_prob.hip against its host twins
(csrc/runtime/svm_prob_cpu.cpp), and the whole family on ``cuda:0`` against ``cpu``."""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.models.base import family_of
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu


def _platt_cases():
    """The 22 machines of tests/test_svc_probability.py: three kinds x seven lengths, and L = 0."""
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


def test_platt_fit_kernel_equals_host_routine():
    cases = _platt_cases()
    n = len(cases)
    assert n == 22
    dec = np.concatenate([c[0] for c in cases])
    lab = np.concatenate([c[1] for c in cases])
    lens = np.array([len(c[0]) for c in cases], np.int64)
    ol = np.ascontiguousarray(np.stack([np.concatenate([[0], np.cumsum(lens)[:-1]]), lens], 1).astype(np.int64))
    AB, st = np.zeros((n, 2)), np.zeros((n, 2), np.int64)
    assert native.cpu_lib().dml_cpu_svm_platt_fit(native.ptr(dec), native.ptr(lab), native.ptr(ol), n,
                                                  native.ptr(AB), native.ptr(st)) == 0
    dev = torch.device("cuda:0")
    d_dec, d_lab, d_ol = (torch.from_numpy(a).to(dev) for a in (dec, lab, ol))
    d_AB = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
    d_st = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
    assert native.hip_lib().dml_svm_platt_fit(native.ptr(d_dec), native.ptr(d_lab), native.ptr(d_ol), n,
                                              native.ptr(d_AB), native.ptr(d_st), native.stream_handle(dev)) == 0
    g_AB, g_st = d_AB.cpu().numpy(), d_st.cpu().numpy()
    print("max |dA|, |dB| =", np.abs(g_AB - AB).max(), "iterations", st[:, 0].tolist())
    assert (g_st == st).all()                       # iterations and status
    assert np.abs(g_AB - AB).max() <= 1e-9
    assert tuple(g_AB[-1]) == (0.0, 0.0) and tuple(g_st[-1]) == (0, 0)     # L = 0: A = B = 0, converged


@pytest.mark.parametrize("k", [2, 3, 5, 64])
def test_pair_proba_kernel_equals_host_routine(k):
    rng = np.random.RandomState(k)
    npairs = k * (k - 1) // 2
    dev = torch.device("cuda:0")
    for m in (1, 63, 65, 1000):
        D = np.ascontiguousarray(2.0 * rng.randn(npairs, m))
        AB = np.ascontiguousarray(np.stack([rng.uniform(-3.0, -0.5, npairs), rng.uniform(-0.5, 0.5, npairs)], 1))
        ref, ref_it = np.empty((m, k)), np.zeros(m, np.int32)
        assert native.cpu_lib().dml_cpu_svm_pair_proba(native.ptr(D), native.ptr(AB), m, k, native.ptr(ref),
                                                       native.ptr(ref_it)) == 0
        d_D, d_AB = torch.from_numpy(D).to(dev), torch.from_numpy(AB).to(dev)
        out = torch.full((m, k), float("nan"), dtype=torch.float64, device=dev)
        its = torch.full((m,), -1, dtype=torch.int32, device=dev)
        assert native.hip_lib().dml_svm_pair_proba(native.ptr(d_D), native.ptr(d_AB), m, k, native.ptr(out),
                                                   native.ptr(its), native.stream_handle(dev)) == 0
        got = out.cpu().numpy()
        print(f"k={k} m={m}: max |gpu - host| = {np.abs(got - ref).max():.3e}, iterations <= {ref_it.max()}")
        assert np.abs(got - ref).max() <= 1e-10
        assert np.abs(got.sum(1) - 1.0).max() <= 1e-12
        assert (its.cpu().numpy() == ref_it).all()


@pytest.mark.parametrize("split", ["1", "0"])
def test_family_log_loss_gpu_matches_cpu(split, monkeypatch):
    """neg_log_loss of the whole family on cuda:0 vs cpu (the data of
    test_svm_gpu_matches_cpu_solver), to the bound that test uses for GPU against host SMO;
    the inner problems ride in the outer problems' launches: 6x the problems, one solve."""
    monkeypatch.setenv("DML_SVM_SPLIT", split)
    rng = np.random.RandomState(5)
    n = 900
    X = rng.randn(n, 6).astype(np.float32)
    y = np.digitize(X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.3 * rng.randn(n), [-0.5, 0.8])   # 3 classes
    fam = family_of("SVC")
    out, problems = {}, {}
    for scoring, flag in (("accuracy", False), ("neg_log_loss", True)):
        grid = [{"C": c, "probability": flag, "random_state": 0} for c in (0.3, 3.0)]
        spec = JobSpec("SVC", grid, cv=3, holdout=False, keep_models="none", scoring=scoring)
        for dev in ("cpu", "cuda:0"):
            res = run_candidates(DeviceData(X, y, True, dev), spec, range(len(grid)))
            assert all(r.ok for r in res), [r.error for r in res]
            assert not any("Platt" in w for r in res for w in r.result.get("warnings", []))
            out[scoring, dev] = np.array([r.result["mean_cv_score"] for r in res])
            problems[scoring, dev] = fam.last_solve_stats["problems"]
    print("neg_log_loss cpu", out["neg_log_loss", "cpu"], "gpu", out["neg_log_loss", "cuda:0"])
    np.testing.assert_allclose(out["neg_log_loss", "cuda:0"], out["neg_log_loss", "cpu"], atol=2e-3)
    assert np.isfinite(out["neg_log_loss", "cuda:0"]).all()
    assert problems["accuracy", "cuda:0"] == 2 * 3 * 3
    assert problems["neg_log_loss", "cuda:0"] == 6 * problems["accuracy", "cuda:0"]
    assert problems["neg_log_loss", "cpu"] == 6 * problems["accuracy", "cpu"]

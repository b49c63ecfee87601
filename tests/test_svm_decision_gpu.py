"""csrc/kernels/svm_decision.hip on the MI355X: the cases of tests/test_svm_decision.py through
the kernels, against the numpy reference and against the host twins; the vote kernel; and the
family with ``DML_SVM_DECISION=1`` against the per-problem loop on ``cuda:0``."""
import ctypes

import numpy as np
import pytest
import torch
from test_svm_decision import (BOUND, CASES, RHO_BRANCHES, check_batch, check_family, check_rho, family_runs,
                               log_loss_scores, make_batch, reference, rho_batch, run_native)

from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernel,svr,shape", CASES)
def test_kernels_against_numpy_and_twins(kernel, svr, shape):
    b = make_batch(kernel, svr, shape)
    gpu, host = run_native(b, "cuda:0"), run_native(b)
    check_batch(b, gpu, f"gpu {kernel} svr={svr} {shape}")
    assert np.array_equal(gpu[1], host[1])                                 # nsv
    for k, n in enumerate(gpu[1]):                                         # compacted indices and coefficients
        r0 = int(b.P[k]["roff"])
        assert np.array_equal(gpu[2][r0:r0 + n], host[2][r0:r0 + n]) and np.array_equal(gpu[3][r0:r0 + n], host[3][r0:r0 + n])
    scale = np.concatenate([np.zeros(0)] + [r[4][np.argsort(b.opos[k])] for k, r in enumerate(reference(b))])
    assert (np.abs(gpu[4] - host[4]) <= BOUND * scale).all()               # exp / tanh differ in the last bits


@pytest.mark.parametrize("case", list(RHO_BRANCHES))
def test_rho_branches_equal_rho(case):
    b = rho_batch(case)
    check_rho(b, run_native(b, "cuda:0")[0])


@pytest.mark.parametrize("nc", [2, 3, 5])
def test_vote_kernel_equals_numpy_vote(nc):
    rng = np.random.RandomState(nc)
    pairs = [(a, b) for a in range(nc) for b in range(a + 1, nc)]
    ms = [1, 65, 300]                                                      # test rows of three fits
    dec = np.round(rng.randn(sum(ms) * len(pairs)), 1)                     # exact zeros among them
    assert (dec == 0).any()
    off, poff, pair_off, want = 0, 0, np.zeros((3, len(pairs)), np.int64), []
    for f, m in enumerate(ms):
        votes = np.zeros((m, nc), np.int64)
        for pi, (a, b) in enumerate(pairs):
            if f == 1 and pi == len(pairs) - 1 and nc > 2:                 # a pair without a machine casts no vote
                pair_off[f, pi] = -1
                continue
            pair_off[f, pi], dv = off, dec[off:off + m]
            votes[:, a] += dv > 0
            votes[:, b] += dv <= 0
            off += m
        want.append(votes.argmax(1))
    fit_tab = np.stack([ms, np.cumsum(ms) - ms], 1).astype(np.int64)
    got = {}
    for dev in ("cpu", "cuda:0"):
        buf = [torch.from_numpy(a).to(dev) for a in (dec, fit_tab, pair_off)] + [torch.full((sum(ms),), -1, dtype=torch.int32, device=dev)]
        args = native.SvmDecArgs(out=native.ptr(buf[0]), fit_tab=native.ptr(buf[1]), pair_off=native.ptr(buf[2]),
                                 pred=native.ptr(buf[3]), F=3, n_classes=nc, max_m=max(ms))
        rc = (native.cpu_lib().dml_cpu_svm_vote(ctypes.byref(args)) if dev == "cpu" else
              native.hip_lib().dml_svm_vote(ctypes.byref(args), native.stream_handle(torch.device(dev))))
        assert rc == 0
        got[dev] = buf[3].cpu().numpy()
    assert np.array_equal(got["cuda:0"], np.concatenate(want)) and np.array_equal(got["cpu"], got["cuda:0"])


@pytest.mark.parametrize("model,n,probability", [("SVC", 900, False), ("SVC", 900, True), ("SVR", 600, False)])
def test_family_batched_path_equals_loop(model, n, probability, monkeypatch):
    """2 C values x cv=3 (``check_family``); the 4-candidate grid takes the same number of launches."""
    stats = check_family(family_runs("cuda:0", model, n, 2, monkeypatch, probability))
    assert stats["launches"] == check_family(family_runs("cuda:0", model, n, 4, monkeypatch, probability))["launches"]


def test_log_loss_scores_agree(monkeypatch):
    assert log_loss_scores("cuda:0", 900, monkeypatch) <= 1e-9

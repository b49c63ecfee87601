"""GradientBoosting stage statistics on the GPU (docs/GBRT_STAGED.md): csrc/kernels/gbrt.hip
k_gb_stage_stats / k_gb_stage_stats_reduce against the host twin (csrc/runtime/
gbrt_stats_cpu.cpp) on the synthetic inputs of test_gbrt_staged.py, and one fit through the fused
stage whose curves are recomputed on the host from the kept model and the fit's own masks.

Counts, squared-error partials and sums are bit-equal to the twin's (the same terms, added in the
same order, contraction off on both sides); the loss sums agree to 1e-12 relative: the device's
and the host's exp / log / log1p differ by ulps, all terms are non-negative.
"""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.model_store import Predictor
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.ops import gbrt_ops

from gbrt_stage_cases import CLS_MIX, LOG, REG_MIX, make_case, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSS_RTOL = 1e-12


def _compare(c):
    got, gpart = run_case(c, DEV)
    ref, rpart = run_case(c, "cpu")
    again, apart = run_case(c, DEV)
    assert got.tobytes() == again.tobytes() and gpart.tobytes() == apart.tobytes()   # two launches, the same bits
    for g, r in ((got, ref), (gpart, rpart)):
        assert (g[..., 0] == r[..., 0]).all()                          # n
        assert (g[..., 1] == r[..., 1]).all()                          # match counts / SSE bits
        gl, rl = g[..., 2].copy().view(np.float64), r[..., 2].copy().view(np.float64)
        assert np.isfinite(gl).all()
        np.testing.assert_allclose(gl, rl, rtol=LOSS_RTOL, atol=0.0)
    assert got[:, 1, :, 0].sum() > 0
    return got


# K = 9 and 70 are above the classes the kernel keeps in registers (8); 70 is also above the 64
# the fused stage handles
@pytest.mark.parametrize("n", [257, 300])
@pytest.mark.parametrize("losses,K", [(CLS_MIX, 1), ([LOG] * 5, 3), ([LOG] * 2, 9), ([LOG], 70), (REG_MIX, 1)])
def test_kernel_equals_the_twin(n, losses, K):
    _compare(make_case(n, K, losses, seed=n + K))


@pytest.mark.parametrize("n", [16 * 256 + 1, 256 * 256 + 1])
@pytest.mark.parametrize("losses", [[LOG, LOG], REG_MIX[:2]])
def test_reduction_levels(n, losses):
    """17 blocks are two levels of the 16-to-1 reduction, 257 blocks three."""
    _compare(make_case(n, 1, losses, seed=5))


@pytest.mark.parametrize("losses,K", [(CLS_MIX, 1), ([LOG] * 2, 3), ([LOG], 9), (REG_MIX, 1)])
@pytest.mark.parametrize("mode", ["big", "ties"])
def test_large_scores_and_exact_ties(losses, K, mode):
    _compare(make_case(300, K, losses, seed=7, mode=mode))


def test_empty_out_of_bag_and_no_validation_mask():
    got = _compare(make_case(300, 1, REG_MIX, seed=3, empty_oob=True, with_val=False))
    assert not got[:, 1, 1].any()
    with_val = _compare(make_case(300, 1, REG_MIX, seed=3, empty_oob=True, with_val=True))
    assert with_val[0, 1, 0, 0] < got[0, 1, 0, 0]                      # fit 0's validation rows left its in-bag rows


def _mean_loss(raw, y):
    z = raw[:, 0]
    return 2.0 * np.mean(np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z))) - y * z)


@pytest.mark.parametrize("subsample", [1.0, 0.5])
def test_fused_fit_curves_equal_a_host_recomputation(subsample):
    rng = np.random.RandomState(4)
    N, D, S = 300, 6, 5
    X = rng.normal(size=(N, D)).astype(np.float32)
    y = (X[:, 0] - X[:, 1] + 0.5 * rng.normal(size=N) > 0).astype(np.int64)
    roles = np.ones((1, N), np.uint8)
    roles[0, ::4] = 2
    dd = DeviceData(X, y, True, DEV)
    dd.set_splits(roles, ["full"])
    fam = family_of("GradientBoostingClassifier")
    rp = fam.resolve("GradientBoostingClassifier", {"n_estimators": S, "subsample": subsample, "random_state": 2},
                     dd.train_counts[0], D, 2)
    out = fam._boost(dd, [FitTask(0, 0, 0, "GradientBoostingClassifier", rp, staged={"scoring": None})], 1, True,
                     want_masks=True)[0]
    torch.cuda.synchronize()
    pr = Predictor(out.model)
    masks = np.asarray(out.info["masks"]).astype(bool)
    train, test = roles[0] == 1, roles[0] == 2
    assert masks.shape == (S, N) and not masks[:, test].any()
    assert (masks.sum(1) == (int(subsample * train.sum()) if subsample < 1 else train.sum())).all()
    raws = list(pr.staged_decision_function(X))
    st = out.info["staged"]
    for s in range(S):
        m = masks[s]
        # the device adds lr * value with one rounding, the host walk with two: 1e-9 covers S adds
        assert pr.train_score_[s] == pytest.approx(_mean_loss(raws[s][m], y[m]), rel=1e-9)
        assert st["train_loss"][s] == pr.train_score_[s]
        assert st["loss"][s] == pytest.approx(_mean_loss(raws[s][test], y[test]), rel=1e-9)
        assert st["score"][s] == np.mean((raws[s][test, 0] >= 0) == y[test])
        if subsample < 1:
            oob = train & ~m
            assert pr.oob_scores_[s] == pytest.approx(_mean_loss(raws[s][oob], y[oob]), rel=1e-9)
    assert out.model["staged_test_score"].tolist() == st["score"]
    if subsample < 1:
        init = np.tile(np.asarray(out.model["init"], dtype=np.float64), (N, 1))
        oob0 = train & ~masks[0]
        assert pr.oob_improvement_[0] == pytest.approx(_mean_loss(init[oob0], y[oob0]) - pr.oob_scores_[0], rel=1e-7)
        assert (pr.oob_improvement_[1:] == pr.oob_scores_[:-1] - pr.oob_scores_[1:]).all()
    else:
        with pytest.raises(AttributeError, match="subsample < 1"):
            pr.oob_scores_
    assert pr.feature_importances_.shape == (D,) and pr.feature_importances_.sum() == pytest.approx(1.0)
    assert pr.feature_importances_[:2].sum() > 0.8

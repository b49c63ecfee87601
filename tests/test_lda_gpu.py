"""csrc/kernels/lda.hip on the GPU against numpy float64, and one job on the GPU data path against
the CPU data path (docs/LDA.md).

Both bounds are rounding bounds, nothing is measured into them: a decision value is a d-term dot
product plus a constant, summed in two orders, so |got - ref| <= 2 (d + 2) 2^-53 (|x|.|w| + |b|); the
Ledoit-Wolf statistic is a sum of n non-negative terms of 2 d + 8 roundings each, so its relative
error is at most (2 d + n + 8) 2^-53 in any order.  The worst ratio to the bound is printed (``-s``).
"""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.ops import lda_ops
from test_lda import LDA, grid, table

pytestmark = pytest.mark.gpu

DS = [1, 15, 16, 17, 33, 128]
U = 2.0 ** -53


@pytest.mark.parametrize("NC", [1, 2, 3, 5, 16, 17])
@pytest.mark.parametrize("C", [2, 3, 17, 64])
@pytest.mark.parametrize("d", DS)
def test_score_matches_numpy(d, C, NC):
    """Five splits of 1, 63, 64, 65 and 200 held-out rows in one launch (a partial row tile, an
    exact one, one row past a tile, four tiles); NC pads to 1, 2, 4, 8 and 16 candidates, and 17 is
    two launches; C = 17 crosses a column tile at NC = 1."""
    rng = np.random.default_rng(7 * d + C)
    n, sizes = 400, [1, 63, 64, 65, 200]
    X = rng.normal(size=(n, d)).astype(np.float32)
    rows = np.concatenate([rng.choice(n, m, replace=False) for m in sizes]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    W, b = rng.normal(size=(len(sizes), C, NC, d)), rng.normal(size=(len(sizes), C, NC))
    parts = [(X[rows[off[s]:off[s + 1]]].astype(np.float64), W[s], b[s].T[:, None, :]) for s in range(len(sizes))]
    ref = np.concatenate([np.einsum("rj,ckj->krc", x, w) + c for x, w, c in parts], 1)
    bound = 2 * (d + 2) * U * np.concatenate([np.einsum("rj,ckj->krc", np.abs(x), np.abs(w)) + np.abs(c)
                                              for x, w, c in parts], 1)
    args = [torch.from_numpy(a).cuda() for a in (X, rows)] + [off] + [torch.from_numpy(a).cuda() for a in (W, b)]
    pred, dec = lda_ops.score(*args, want_dec=True)
    pred_only, none = lda_ops.score(*args)
    ratio = float((np.abs(dec.cpu().numpy() - ref) / bound).max())
    print(f"kernel vs numpy at d={d} C={C} NC={NC}: {ratio:.3f} of the bound")
    assert dec.shape == ref.shape and ratio <= 1.0
    top = np.sort(ref, -1)
    clear = (top[..., -1] - top[..., -2]) > 2 * bound.max(-1)
    assert clear.mean() >= 0.9
    assert (pred.cpu().numpy()[clear] == ref.argmax(-1)[clear]).all()
    assert none is None and torch.equal(pred_only, pred)


@pytest.mark.parametrize("NC", [1, 2, 4])
@pytest.mark.parametrize("lo,hi", [(3, 20), (4, 23)])
def test_score_ties_keep_the_lower_class(lo, hi, NC):
    """Classes lo and hi share their rows of W and b and beat every other class: their columns
    lo * NC + k and hi * NC + k lie in different column tiles and, for NC = 1 and 2, in different
    lane groups (column mod 4), the lower class once in the higher group and once in the lower."""
    rng = np.random.default_rng(lo)
    d, C, m = 17, 24, 70
    X = torch.from_numpy(rng.normal(size=(m, d)).astype(np.float32)).cuda()
    W, b = np.zeros((1, C, NC, d)), np.full((1, C, NC), -1e30)
    W[0, lo] = W[0, hi] = rng.normal(size=(NC, d))
    b[0, lo] = b[0, hi] = rng.normal(size=NC)
    pred, dec = lda_ops.score(X, torch.arange(m), [0, m], torch.from_numpy(W), torch.from_numpy(b), want_dec=True)
    assert torch.equal(dec[..., lo], dec[..., hi]) and (pred == lo).all()


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", [257, 1030])
def test_lw_stat_matches_numpy_and_repeats(n, d):
    """Cells = 4 fold buckets (3 splits and the never-held-out rows) x 3 classes; cell (3, 0) is
    empty and cell (2, 1) holds one row; 3 partitions, so a cell's row blocks are spread over them."""
    rng = np.random.default_rng(n + d)
    C, S = 3, 3
    X = (rng.normal(size=(n, d)) * 3 + 1.5).astype(np.float32)
    y, bk = rng.integers(0, C, n), rng.integers(0, 4, n)
    bk[(bk == 3) & (y == 0)] = 0
    bk[np.nonzero((bk == 2) & (y == 1))[0][1:]] = 1
    cell = bk * C + y
    counts = np.bincount(cell, minlength=4 * C)
    assert counts[3 * C] == 0 and counts[2 * C + 1] == 1
    train = np.arange(4)[:, None] != np.arange(S)[None, :]            # bucket s is held out in split s
    mean, w = rng.normal(size=(S, C, d)) + 1.5, rng.uniform(0.05, 0.2, size=(S, C, d))
    q = np.einsum("nsj,nsj->ns", (X.astype(np.float64)[:, None, :] - mean[:, y].transpose(1, 0, 2)) ** 2, w[:, y].transpose(1, 0, 2))
    ref = np.stack([(q[cell == k] ** 2).sum(0) for k in range(4 * C)]) * np.repeat(train, C, 0)
    args = (torch.from_numpy(X).cuda(), torch.from_numpy(np.argsort(cell, kind="stable").astype(np.int32)),
            torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])), torch.from_numpy(train),
            torch.from_numpy(mean), torch.from_numpy(w))
    got = lda_ops.lw_stat(*args, parts=3)
    err = np.abs(got.cpu().numpy() - ref)
    print(f"lw_stat vs numpy at n={n} d={d}: {float((err / np.maximum(ref, 1e-300)).max() / ((2 * d + n + 8) * U)):.3f} of the bound")
    assert (err <= (2 * d + n + 8) * U * ref).all()
    assert torch.equal(lda_ops.lw_stat(*args, parts=3), got)


def test_job_on_gpu_matches_cpu_path():
    X, y = table(200, 17, 4)
    g = grid(4)
    acc = lambda dev: [r.result["cv_scores"] for r in run_candidates(
        DeviceData(X, y, True, dev), JobSpec(LDA, g, cv=3, holdout=True), range(len(g)))]
    # the same correct counts: the GPU path's batched accuracy is a device mean, the CPU path's a
    # host division, so a score may differ in its last place (2 roundings, against 1 / 67 per row)
    np.testing.assert_allclose(acc("cuda"), acc("cpu"), rtol=4 * np.finfo(np.float64).eps, atol=0)


def test_limits_are_reported_not_launched():
    X = torch.zeros((4, 129), dtype=torch.float32, device="cuda")
    with pytest.raises(lda_ops.LdaTooLarge):
        lda_ops.score(X, torch.arange(4), [0, 4], torch.zeros((1, 2, 1, 129)), torch.zeros((1, 2, 1)))
    with pytest.raises(lda_ops.LdaTooLarge):
        lda_ops.lw_stat(X, torch.arange(4), torch.tensor([0, 2, 4]), torch.ones((1, 1)), torch.zeros((1, 2, 129)),
                        torch.ones((1, 2, 129)))
    assert lda_ops.max_d() >= 128 and lda_ops.max_candidates() >= 16

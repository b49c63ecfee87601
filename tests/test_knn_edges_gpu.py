"""KNN kernels (csrc/kernels/neighbors.hip) where they can go wrong unnoticed: tables far
from the origin or in far-apart clusters (the matrix-core path selects by an approximate
distance), exact-arithmetic lattices full of ties, tile / K-step boundaries, fewer training
rows than K.  The reference everywhere is ``knn_search_torch`` on ``X.double()``; "strictly
equal" means equal indices AND bit-equal float32 accumulators between the matrix-core path
and the scalar kernel (``DML_KNN_MFMA=0``)."""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.models import neighbors as nb
from test_knn_select import KINDS, N_QUERIES, N_ROWS, Table, knn_inputs, two_split_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _search(tab, K, metric, p, mfma, monkeypatch):
    """(results per split, stats) of one ``knn_search_hip`` call on the chosen L2 path."""
    monkeypatch.setenv("DML_KNN_MFMA", "1" if mfma else "0")
    got = nb.knn_search_hip(tab, sorted(tab.test_rows), K, metric, p)
    return got, dict(nb.last_search_stats)


def _assert_strictly_equal(a, b):
    assert sorted(a) == sorted(b)
    for s in a:
        assert torch.equal(a[s][1], b[s][1]), f"split {s}: neighbour ids differ"
        assert torch.equal(a[s][0], b[s][0]), f"split {s}: accumulators differ"


def _reference(tab, K, metric, p):
    Xd = tab.X.double()
    return {s: nb.knn_search_torch(Xd, tab.test_rows[s], tab.train_rows(s), K, metric, p) for s in tab.test_rows}


def _assert_matches_reference(got, ref, K, exact=False):
    """The rule of ``test_knn_kernel_matches_torch`` on the first min(K, n_train) slots
    (``exact``: equality, no escape); the slots past the training rows hold -1 / +inf."""
    for s, (ref_d, ref_i) in ref.items():
        gd, gi = got[s]
        assert gd.shape == (ref_d.shape[0], K) and gi.shape == gd.shape
        k = ref_d.shape[1]                                  # min(K, n_train)
        assert bool((gi[:, k:] == -1).all()) and bool(torch.isposinf(gd[:, k:]).all())
        gd, gi = gd[:, :k].double(), gi[:, :k]
        if exact:
            assert torch.equal(gi, ref_i) and torch.equal(gd, ref_d)
            continue
        if k == 0:
            continue
        scale = max(1.0, float(ref_d.median()))
        torch.testing.assert_close(gd, ref_d, rtol=2e-5, atol=1e-5 * scale)
        mismatch = gi != ref_i
        if mismatch.any():   # only where two distances are within float32 round-off
            close = (ref_d[mismatch] - gd[mismatch]).abs() <= 1e-4 * ref_d[mismatch].abs().clamp_min(1)
            assert bool(close.all())


# ---- a. off-origin and clustered tables ------------------------------------------------
_REF32 = {}


def _offorigin(kind, d):
    """(table, float64 reference at K = 32) -- built once per (kind, d); the K nearest are a
    prefix of the 32 nearest."""
    if (kind, d) not in _REF32:
        tab = two_split_table(knn_inputs(kind, N_ROWS, d), DEV)
        _REF32[kind, d] = (tab, _reference(tab, 32, nb.M_L2, 2.0))
    return _REF32[kind, d]


@pytest.mark.parametrize("K", [1, 5, 32])
@pytest.mark.parametrize("d", [4, 10, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_l2_search_off_origin(kind, d, K, monkeypatch):
    tab, ref32 = _offorigin(kind, d)
    ref = {s: (rd[:, :K], ri[:, :K]) for s, (rd, ri) in ref32.items()}
    mf, stats = _search(tab, K, nb.M_L2, 2.0, True, monkeypatch)
    sc, _ = _search(tab, K, nb.M_L2, 2.0, False, monkeypatch)
    print(f"{kind} d={d} K={K}: {stats}")
    _assert_strictly_equal(mf, sc)
    _assert_matches_reference(sc, ref, K)
    _assert_matches_reference(mf, ref, K)
    # neither path may hide behind the other: the matrix cores do the work on centred,
    # scaled and shifted tables, the scalar fallback runs on two far clusters
    assert stats["mfma_queries"] == 2 * N_QUERIES
    if kind in ("randn", "scaled", "plus500"):
        assert stats["fallback_queries"] == 0
    if kind == "pm500":
        assert stats["fallback_queries"] > 0


# ---- b. exact-arithmetic lattice --------------------------------------------------------
def _lattice(d):
    rng = np.random.RandomState(d)
    X = rng.randint(-3, 4, size=(700, d)).astype(np.float32)
    roles = np.zeros((1, 700), np.uint8)
    roles[0, 100:] = 1
    return Table(X, roles, [np.arange(100)], DEV)


@pytest.mark.parametrize("metric,p", [(nb.M_L2, 2.0), (nb.M_L1, 1.0), (nb.M_LINF, float("inf"))])
@pytest.mark.parametrize("K", [1, 7, 32, 64])
@pytest.mark.parametrize("d", [1, 4, 16])
def test_integer_lattice_is_exact(d, K, metric, p, monkeypatch):
    """Integers in [-3, 3]: every accumulator is exact in float32, so distances and ids equal
    the float64 reference outright, ties (lower row id first) included.  At d = 1 each query
    has >= 64 training rows at distance 0: the 64-candidate window is all exact ties, which
    the matrix-core kernel must not certify."""
    tab = _lattice(d)
    ref = _reference(tab, K, metric, p)
    if d == 1:
        zero = (tab.X[:100, None, 0] == tab.X[None, 100:, 0]).sum(1)
        assert int(zero.min()) >= 64
    sc, _ = _search(tab, K, metric, p, False, monkeypatch)
    _assert_matches_reference(sc, ref, K, exact=True)
    if metric == nb.M_L2 and K <= nb.MFMA_KMAX:
        mf, stats = _search(tab, K, metric, p, True, monkeypatch)
        _assert_matches_reference(mf, ref, K, exact=True)
        assert stats["mfma_queries"] == 100
        if d == 1:
            assert stats["fallback_queries"] > 0


# ---- c. tile and K-step edges -----------------------------------------------------------
def _edge_table(n, d, layout):
    """Two splits with 13 and 24 queries (not multiples of 8 / of 32).  ``head``: training
    rows [24, n), every second one for split 1.  ``tail``: training rows only in the last
    partial batch of 64 rows."""
    X = np.random.RandomState(1000 * n + d).randn(n, d).astype(np.float32)
    roles = np.zeros((2, n), np.uint8)
    if layout == "head":
        roles[0, 24:] = 1
        roles[1, 24::2] = 1
    else:
        assert n % 64
        roles[:, n - n % 64:] = 1
    return Table(X, roles, [np.arange(13), np.arange(24)], DEV)


@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("n,d,layout", [
    (64, 1, "head"), (64, 100, "head"), (128, 16, "head"), (128, 129, "head"), (129, 17, "head"),
    (129, 128, "tail"), (129, 16, "tail"), (191, 100, "tail"), (191, 1, "head"), (191, 129, "head"),
    (256, 128, "head"), (256, 17, "head")])
def test_tile_and_kstep_edges(n, d, layout, K, monkeypatch):
    """Row counts at and around the 64-row batch and the 128-row tile; d of 1, 16, 17, 100,
    128, 129 gives 1, 1, 2, 8, 8 and 9 K-steps (9 streams the query operand)."""
    tab = _edge_table(n, d, layout)
    assert nb.mfma_operands(tab)[2] == {1: 1, 16: 1, 17: 2, 100: 8, 128: 8, 129: 9}[d]
    mf, stats = _search(tab, K, nb.M_L2, 2.0, True, monkeypatch)
    sc, _ = _search(tab, K, nb.M_L2, 2.0, False, monkeypatch)
    assert stats["mfma_queries"] == 37
    _assert_strictly_equal(mf, sc)
    _assert_matches_reference(sc, _reference(tab, K, nb.M_L2, 2.0), K)


# ---- d. fewer training rows than K ------------------------------------------------------
@pytest.mark.parametrize("K,mfma", [(64, False), (32, True)])
def test_fewer_training_rows_than_k(K, mfma, monkeypatch):
    """40 training rows in split 0, none in split 1: the first min(K, n_train) slots equal
    the reference, the rest hold id -1 and distance +inf."""
    X = np.random.RandomState(5).randn(100, 5).astype(np.float32)
    roles = np.zeros((2, 100), np.uint8)
    roles[0, 60:] = 1
    tab = Table(X, roles, [np.arange(20), np.arange(20)], DEV)
    got, stats = _search(tab, K, nb.M_L2, 2.0, mfma, monkeypatch)
    assert stats["mfma_queries"] == (40 if mfma else 0)
    ref = _reference(tab, K, nb.M_L2, 2.0)
    assert ref[0][0].shape[1] == min(K, 40) and ref[1][0].shape[1] == 0
    _assert_matches_reference(got, ref, K)


# ---- e. end to end ----------------------------------------------------------------------
def test_knn_grid_off_origin_matches_cpu():
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
    from cs230_distributed_machine_learning_amd.search.grid import ParameterGrid

    rng = np.random.RandomState(0)
    X = (rng.randn(1500, 4) + 500).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] > 750).astype(int)
    grid = list(ParameterGrid({"n_neighbors": [1, 5], "weights": ["uniform", "distance"]}))
    out = {}
    for dev in ("cpu", DEV):
        dd = DeviceData(X, y, True, dev)
        res = run_candidates(dd, JobSpec("KNeighborsClassifier", grid, cv=5), range(len(grid)))
        assert all(r.ok for r in res), [r.error for r in res]
        out[dev] = np.array([r.result["mean_cv_score"] for r in res])
    np.testing.assert_allclose(out[DEV], out["cpu"], atol=1e-3)

"""neighbors_wide.hip and the cosine metric against ``knn_search_torch`` on ``X.double()``."""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.models import neighbors as nb
from test_knn_select import Table, knn_inputs, two_split_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METRICS = {"l2": (nb.M_L2, 2.0), "l1": (nb.M_L1, 1.0), "linf": (nb.M_LINF, float("inf")), "p3": (nb.M_P, 3.0)}


def _search(tab, K, metric, p, wide, monkeypatch):
    monkeypatch.setenv("DML_KNN_MFMA", "0")
    monkeypatch.setenv("DML_KNN_WIDE", wide)
    got = nb.knn_search_hip(tab, sorted(tab.test_rows), K, metric, p)
    return got, dict(nb.last_search_stats)


def _reference(tab, K, metric, p):
    Xd, q = tab.X.double(), tab.test_rows
    return {s: nb.knn_search_torch(Xd, q[s], tab.train_rows(s), K, metric, p) for s in q}


def _assert_matches_reference(got, ref, K, exact=False):
    """Returns the share of id slots that used the near-tie escape (``exact``: no escape)."""
    escaped = slots = 0
    for s, (ref_d, ref_i) in ref.items():
        gd, gi = got[s]
        assert gd.shape == (ref_d.shape[0], K) and gi.shape == gd.shape
        k = ref_d.shape[1]                                  # min(K, n_train)
        assert bool((gi[:, k:] == -1).all()) and bool(torch.isposinf(gd[:, k:]).all())
        gd, gi = gd[:, :k].double(), gi[:, :k]
        if exact:
            assert torch.equal(gi, ref_i) and torch.equal(gd, ref_d)
        if exact or k == 0:
            continue
        scale = max(1.0, float(ref_d.median()))
        torch.testing.assert_close(gd, ref_d, rtol=2e-5, atol=1e-5 * scale)
        mismatch = gi != ref_i
        # ids may differ only where two distances are within float32 round-off
        assert bool(((ref_d - gd).abs() <= 1e-4 * ref_d.abs().clamp_min(1))[mismatch].all())
        escaped, slots = escaped + int(mismatch.sum()), slots + mismatch.numel()
    return escaped / max(1, slots)


@pytest.mark.parametrize("K", [1, 7, 64])
@pytest.mark.parametrize("d", [4, 33])
@pytest.mark.parametrize("name", list(METRICS))
def test_wide_equals_narrow(name, d, K, monkeypatch):
    metric, p = METRICS[name]
    tab = two_split_table(knn_inputs("randn", 1500, d), DEV)
    wide, stats = _search(tab, K, metric, p, "1", monkeypatch)
    narrow, nstats = _search(tab, K, metric, p, "0", monkeypatch)
    assert stats["wide_queries"] == 512 and nstats["wide_queries"] == 0
    for s in narrow:   # equal ids, bit-equal accumulators
        assert torch.equal(wide[s][1], narrow[s][1]) and torch.equal(wide[s][0], narrow[s][0])


@pytest.mark.parametrize("name", ["l2", "l1", "linf"])
@pytest.mark.parametrize("K", [65, 128, 200, 512])
@pytest.mark.parametrize("d", [1, 4])
def test_integer_lattice_is_exact(d, K, name, monkeypatch):
    """Exact float32 accumulators; at d = 1 the K-th slot of every query lies inside a block
    of equal distances, so the lower-row-id rule decides which rows are kept."""
    X = np.random.RandomState(d).randint(-3, 4, size=(700, d)).astype(np.float32)
    roles = (np.arange(700) >= 100)[None].astype(np.uint8)
    tab = Table(X, roles, [np.arange(100)], DEV)
    if d == 1:
        D = np.sort(np.abs(X[:100, 0][:, None] - X[100:, 0][None, :]), axis=1)
        assert (D[:, K - 1] == D[:, K]).all()
    metric, p = METRICS[name]
    got, stats = _search(tab, K, metric, p, "auto", monkeypatch)
    assert stats["wide_queries"] == 100
    _assert_matches_reference(got, _reference(tab, K, metric, p), K, exact=True)


@pytest.mark.parametrize("K", [65, 512])
@pytest.mark.parametrize("n", [577, 1100])
def test_worst_case_arrival_order(n, K, monkeypatch):
    """Queries at 0..15, training rows at n + 20 - row: every row beats all rows before it."""
    X = np.concatenate([np.arange(16), n + 20 - np.arange(16, n)]).astype(np.float32)[:, None]
    roles = (np.arange(n) >= 16)[None].astype(np.uint8)
    tab = Table(X, roles, [np.arange(16)], DEV)
    got, _ = _search(tab, K, nb.M_L2, 2.0, "auto", monkeypatch)
    _assert_matches_reference(got, _reference(tab, K, nb.M_L2, 2.0), K, exact=True)


@pytest.mark.parametrize("layout,n,K", [("head", 300, 100), ("tail", 300, 100), ("few", 100, 128)])
def test_edges(layout, n, K, monkeypatch):
    """13 and 24 queries.  ``head``: split 1 trains on every second row of split 0's; ``tail``:
    only the last partial 64-row batch trains; ``few``: 40 training rows in split 0, none in 1."""
    X = np.random.RandomState(n + K).randn(n, 5).astype(np.float32)
    roles = np.zeros((2, n), np.uint8)
    if layout == "head":
        roles[0, 24:] = 1
        roles[1, 24::2] = 1
    elif layout == "tail":
        roles[:, n - n % 64:] = 1
    else:
        roles[0, 60:] = 1
    tab = Table(X, roles, [np.arange(13), np.arange(24)], DEV)
    ref = _reference(tab, K, nb.M_L2, 2.0)
    assert ref[1][0].shape[1] == {"head": K, "tail": n % 64, "few": 0}[layout]
    got, stats = _search(tab, K, nb.M_L2, 2.0, "auto", monkeypatch)
    assert stats["wide_queries"] == 37
    _assert_matches_reference(got, ref, K)


@pytest.mark.parametrize("K", [5, 64, 100])
@pytest.mark.parametrize("d", [4, 33])
@pytest.mark.parametrize("kind", ["randn", "plus500"])
def test_cosine(kind, d, K, monkeypatch):
    """Zero rows among queries and training rows.  The escape cap holds for ``randn`` only: rows
    of ``plus500`` are all but parallel, their distances (~1e-6) lie at float32's resolution of
    1 - cos, and float32 ``knn_search_torch`` itself escapes on 60 to 92 % of the slots there."""
    X = knn_inputs(kind, 1500, d)
    X[[0, 1, 2, 3, 4, 300, 301, 302, 303, 304]] = 0.0
    tab = two_split_table(X, DEV)
    got, stats = _search(tab, K, nb.M_COS, 0.0, "auto", monkeypatch)
    assert stats["wide_queries"] == (512 if K > 64 else 0)
    escaped = _assert_matches_reference(got, _reference(tab, K, nb.M_COS, 0.0), K)
    assert escaped <= 0.01 or kind == "plus500"


def test_knn_grid_wide_and_cosine_matches_cpu():
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
    from cs230_distributed_machine_learning_amd.search.grid import ParameterGrid
    X = np.random.RandomState(0).randn(1500, 4).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] > 0).astype(int)
    grid = list(ParameterGrid({"n_neighbors": [5, 100], "weights": ["uniform", "distance"],
                               "metric": ["minkowski", "cosine"]}))
    out = {}
    for dev in ("cpu", DEV):
        dd = DeviceData(X, y, True, dev)
        res = run_candidates(dd, JobSpec("KNeighborsClassifier", grid, cv=5), range(len(grid)))
        assert all(r.ok for r in res), [r.error for r in res]
        out[dev] = np.array([r.result["mean_cv_score"] for r in res])
    np.testing.assert_allclose(out[DEV], out["cpu"], atol=1e-3)
    assert nb.last_search_stats["wide_queries"] > 0

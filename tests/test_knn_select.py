"""The matrix-core KNN search's selection error bound, checked on the CPU.

``k_knn_l2_mfma`` (csrc/kernels/neighbors.hip) ranks candidates by a bf16x3 approximation
of ``||q - r||^2`` built from ``mfma_operands``' output, and certifies a query only if its
exact K-th distance lies more than ``eps(q)`` below the largest approximate distance it
kept.  That is sound only if ``eps(q)`` really bounds the approximation's error, on data
far from the origin too.  Here the approximate distance is emulated in torch from the very
operands the kernel reads (same hi/lo planes, fp32 accumulation; the accumulation order
differs from the hardware's, the bound charges every addition) and compared with float64.

The input families and the stub table are shared with tests/test_knn_edges_gpu.py.
"""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.models import neighbors as nb

KINDS = ("randn", "scaled", "plus500", "pm500", "bernoulli", "big")
N_ROWS, N_QUERIES = 1500, 256


def knn_inputs(kind: str, n: int, d: int, seed: int = 0) -> np.ndarray:
    """float32 [n, d] tables: centred, per-column scales, off-origin, two clusters, one
    huge binary column, large offset with large scale."""
    rng = np.random.RandomState(1000 * seed + 17 * d + KINDS.index(kind))
    X = rng.randn(n, d)
    if kind == "scaled":
        X = X * rng.uniform(0.1, 10, d)
    elif kind == "plus500":
        X = X + 500
    elif kind == "pm500":
        X = X + 500 * np.where(rng.rand(n, 1) < 0.5, -1.0, 1.0)
    elif kind == "bernoulli":
        X[:, -1] = 1000.0 * (rng.rand(n) < 0.5)
    elif kind == "big":
        X = X * 1000 + 1e5
    return X.astype(np.float32)


class Table:
    """The attributes ``knn_search_hip`` reads (those of ``_QueryTable``), with hand-written
    role rows: roles[s, j] == 1 makes row j a TRAIN row of split s; ``queries[s]`` are the
    rows searched for split s."""

    def __init__(self, X, roles, queries, device="cpu"):
        self.device = torch.device(device)
        self.X = torch.as_tensor(X, dtype=torch.float32).contiguous().to(self.device)
        self.n, self.d = int(self.X.shape[0]), int(self.X.shape[1])
        self.roles = torch.as_tensor(np.asarray(roles), dtype=torch.uint8).contiguous().to(self.device)
        self.test_rows = {s: torch.as_tensor(np.asarray(q), dtype=torch.int32).to(self.device)
                          for s, q in enumerate(queries)}

    def train_rows(self, s):
        return torch.nonzero(self.roles[s] == 1).flatten()

    def feature_major(self):
        if getattr(self, "_XT", None) is None:
            self._XT = self.X.t().contiguous()
        return self._XT


def two_split_table(X, device="cpu"):
    """Rows [0, 256) are the queries of both splits; split 0 trains on every other row,
    split 1 on a different subset (every third of them dropped), so the split index matters."""
    n = X.shape[0]
    roles = np.zeros((2, n), dtype=np.uint8)
    roles[0, N_QUERIES:] = 1
    roles[1, N_QUERIES:] = (np.arange(N_QUERIES, n) % 3 != 0)
    return Table(X, roles, [np.arange(N_QUERIES), np.arange(N_QUERIES)], device)


def _planes(ops):
    xhl, npad, ks = ops[0], ops[1], ops[2]
    hi, lo = (xhl[i].transpose(0, 1).reshape(npad, ks * 16).float() for i in (0, 1))
    return hi, lo


def _approx(ops, n):
    """The kernel's approximate squared distances [256 queries, n rows], and eps per query."""
    hi, lo = _planes(ops)
    rn, rmax, c1, c2 = ops[3], ops[4], ops[5], ops[6]
    qh, ql, rh, rl = hi[:N_QUERIES], lo[:N_QUERIES], hi[:n], lo[:n]
    acc = ql @ rh.t() + qh @ rl.t() + qh @ rh.t()
    approx = (rn[:N_QUERIES, None] + rn[None, :n] - 2.0 * acc).clamp_min(0.0)
    f = lambda v: torch.tensor(v, dtype=torch.float32)   # the kernel evaluates eps in float32
    eps = nb.mfma_error_bound(rn[:N_QUERIES], f(rmax), f(c1), f(c2))
    assert approx.dtype == torch.float32 and eps.dtype == torch.float32
    return approx, eps


@pytest.mark.parametrize("d", [4, 10, 33, 150])
@pytest.mark.parametrize("kind", KINDS)
def test_error_bound_holds_for_every_pair(kind, d):
    X = knn_inputs(kind, N_ROWS, d)
    tab = Table(X, np.zeros((1, N_ROWS), np.uint8), [np.arange(N_QUERIES)])
    approx, eps = _approx(nb.mfma_operands(tab), N_ROWS)
    Xd = tab.X.double()
    exact = torch.cdist(Xd[:N_QUERIES], Xd, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    ratio = ((approx.double() - exact).abs() / eps.double()[:, None]).max().item()
    print(f"{kind} d={d}: max |approx - exact| / eps = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("d", [4, 10, 33])
def test_operands_are_translation_consistent(d):
    """Operands of X and of X + 512 describe the same centred table up to rounding: 2^-15 for
    the float32 rounding of each shifted entry (|x + 512| < 1024), as much for the shift of
    the column mean that causes, and per side 2^-24 |a| for the centred row's own rounding
    and 2^-18 |a| for what the hi/lo split drops."""
    X = knn_inputs("randn", N_ROWS, d)
    tabs = [Table(A, np.zeros((1, N_ROWS), np.uint8), [np.arange(1)]) for A in (X, X + np.float32(512))]
    a, b = (nb.mfma_operands(t) for t in tabs)
    (ha, la), (hb, lb) = _planes(a), _planes(b)
    xa, xb = (ha.double() + la.double())[:N_ROWS], (hb.double() + lb.double())[:N_ROWS]
    amax = xa.abs().max().item()
    tol = 2.0 ** -14 + 2 * (2.0 ** -18 + 2.0 ** -24) * amax
    assert (xa - xb).abs().max().item() <= tol
    assert not xa[:, d:].any() and not xb[:, d:].any()          # feature padding stays zero
    rna, rnb = a[3].double(), b[3].double()
    # |a|^2 moves by at most 2 |a| sqrt(d) 2^-14 + d 2^-28, plus one float32 rounding per side
    assert bool(((rna - rnb).abs() <= 2 * rna.sqrt() * d ** 0.5 * 2.0 ** -14 + d * 2.0 ** -28 + 2.0 ** -22 * rna).all())
    assert abs(a[4] - b[4]) <= 2.0 ** -12 * a[4]               # rmax


def _emulated_search(X, K):
    """Selection, re-rank and certificate of the kernel, emulated; returns (certified [q],
    re-ranked ids [q, K], full-search ids [q, K]) for split 0 of ``two_split_table``."""
    tab = two_split_table(X)
    approx, eps = _approx(nb.mfma_operands(tab), N_ROWS)
    tr = tab.train_rows(0)
    A = approx[:, tr]
    As, order = torch.sort(A, dim=1, stable=True)
    cand = order[:, :64]                                           # columns of ``tr``, ascending row id on ties
    a64 = As[:, 63]
    D = ((tab.X[tr][None, :, :] - tab.X[:N_QUERIES][:, None, :]) ** 2).sum(2)   # float32, like the re-rank
    cand_sorted = torch.sort(cand, dim=1).values
    Dc, oc = torch.sort(D.gather(1, cand_sorted), dim=1, stable=True)
    got = tr[cand_sorted.gather(1, oc[:, :K])]
    dK = Dc[:, K - 1]
    lim = (a64 - eps) * (1.0 - (tab.d + 6) * 2.0 ** -24)
    full = tr[torch.sort(D, dim=1, stable=True).indices[:, :K]]
    return dK < lim, got, full


@pytest.mark.parametrize("K", [1, 5, 32])
@pytest.mark.parametrize("d", [4, 10, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_emulated_certificate(kind, d, K):
    """A certified query's re-ranked neighbours are the full search's, and the data decide
    which path works: centred, scaled and shifted tables certify every query, two far
    clusters do not."""
    cert, got, full = _emulated_search(knn_inputs(kind, N_ROWS, d), K)
    assert torch.equal(got[cert], full[cert])
    uncertified = int((~cert).sum())
    print(f"{kind} d={d} K={K}: {uncertified} of {N_QUERIES} uncertified")
    if kind in ("randn", "scaled", "plus500"):
        assert uncertified == 0
    if kind == "pm500":
        assert uncertified > 0

"""Shared fixtures of the Lasso / ElasticNet solver tests (test_enet.py, test_enet_gpu.py); no
test functions.

Seeded float32 tables with n = 400 rows, used as their float64 copies: d in {1, 3, 63, 64, 65,
130} (below, at and above one wave's 64 lanes; more than two entries per lane), one column
constant, sparse true coefficients.  Every table is crossed with alpha in {1e-3, 0.05, 0.5, 1e3}
(the last is above alpha_max: the w_max == 0 exit in sweep 1), l1_ratio in {1, 0.5, 0}, positive
in {False, True} and (max_iter, tol) in {(1000, 1e-4), (2, 1e-4), (100000, 1e-10)} (the middle
pair ends unconverged through the last-sweep gap check): 6 x 72 = 432 problems on 6 Grams.

A problem is (Q, q, y) built in numpy float64 from the centred rows, as sklearn builds its
precomputed Gram, plus sklearn's ``l1_reg = alpha * l1_ratio * n`` and
``l2_reg = alpha * (1 - l1_ratio) * n``.  ``solver_inputs(d)`` gives one d's problems on its
own Gram, ``batched_inputs()`` all of them as one batch on six Grams."""
import itertools
from functools import lru_cache

import numpy as np

N = 400
DS = (1, 3, 63, 64, 65, 130)
ALPHAS = (1e-3, 0.05, 0.5, 1e3)
L1_RATIOS = (1.0, 0.5, 0.0)
POSITIVE = (False, True)
ITER_TOL = ((1000, 1e-4), (2, 1e-4), (100000, 1e-10))
# seed of every table; a seed is replaced (and test_enet.py says so) only when a case sits on a
# rounding threshold of the d_w_max / w_max < tol test
SEEDS = {1: 101, 3: 103, 63: 163, 64: 164, 65: 165, 130: 230}


def table(d: int, seed: int = None):
    """(X float32 [N, d], y float32 [N]): column min(2, d - 1) constant unless d == 1, about
    a fifth of the true coefficients nonzero."""
    rng = np.random.RandomState(SEEDS[d] if seed is None else seed)
    X = rng.normal(size=(N, d)).astype(np.float32)
    X[:, : d // 2] += (0.5 * rng.normal(size=(N, 1))).astype(np.float32)   # correlated columns
    if d > 1:
        X[:, min(2, d - 1)] = 1.5
    coef = np.zeros(d)
    nz = rng.choice(d, size=max(1, d // 5), replace=False)
    coef[nz] = rng.normal(size=len(nz)) * 2.0
    y = (X.astype(np.float64) @ coef + 0.5 + 0.3 * rng.normal(size=N)).astype(np.float32)
    return X, y


@lru_cache(maxsize=None)
def gram(d: int):
    """(Q [d, d], q [d], yc [N]) float64 of the centred table, as sklearn's ``_pre_fit`` does."""
    X, y = table(d)
    Xc = X.astype(np.float64)
    Xc = Xc - Xc.mean(0)
    yc = y.astype(np.float64)
    yc = yc - yc.mean()
    Q = np.ascontiguousarray(Xc.T @ Xc)
    for m in (Q,):
        m.setflags(write=False)
    q = Xc.T @ yc
    q.setflags(write=False)
    yc.setflags(write=False)
    return Q, q, yc


@lru_cache(maxsize=None)
def problems():
    """Every case as a dict: d, g (index into DS), alpha, l1_ratio, positive, max_iter, tol,
    l1, l2 -- problems of different Grams interleaved (the Gram index varies fastest)."""
    out = []
    for alpha, l1r, pos, (mi, tol) in itertools.product(ALPHAS, L1_RATIOS, POSITIVE, ITER_TOL):
        for g, d in enumerate(DS):
            out.append({"d": d, "g": g, "alpha": alpha, "l1_ratio": l1r, "positive": pos, "max_iter": mi, "tol": tol,
                        "l1": alpha * l1r * N, "l2": alpha * (1.0 - l1r) * N})
    return tuple(out)


def solver_inputs(d: int):
    """The problems of one d as the arrays ``ops.enet_ops.enet_cd`` takes (numpy, one Gram)."""
    Q, q, yc = gram(d)
    ps = [p for p in problems() if p["d"] == d]
    return {
        "Q": Q[None], "q": q[None], "ynorm2": np.array([yc @ yc]),
        "gram_id": np.zeros(len(ps), dtype=np.int32),
        "l1": np.array([p["l1"] for p in ps]), "l2": np.array([p["l2"] for p in ps]),
        "positive": np.array([int(p["positive"]) for p in ps], dtype=np.int32),
        "max_iter": np.array([p["max_iter"] for p in ps], dtype=np.int32),
        "tol": np.array([p["tol"] for p in ps]),
    }, ps


@lru_cache(maxsize=None)
def batched_inputs():
    """Every problem of every d as ONE batch for ``enet_cd``: the six Grams zero-padded to the
    largest d (a padded coordinate has a zero diagonal, so the solver skips it; it is a column of
    zeros appended to the table) and the problems in ``problems()`` order, so consecutive
    problems sit on different Grams."""
    dmax = max(DS)
    Q = np.zeros((len(DS), dmax, dmax))
    q = np.zeros((len(DS), dmax))
    yn = np.zeros(len(DS))
    for g, d in enumerate(DS):
        Qg, qg, yc = gram(d)
        Q[g, :d, :d] = Qg
        q[g, :d] = qg
        yn[g] = yc @ yc
    ps = problems()
    return {
        "Q": Q, "q": q, "ynorm2": yn,
        "gram_id": np.array([p["g"] for p in ps], dtype=np.int32),
        "l1": np.array([p["l1"] for p in ps]), "l2": np.array([p["l2"] for p in ps]),
        "positive": np.array([int(p["positive"]) for p in ps], dtype=np.int32),
        "max_iter": np.array([p["max_iter"] for p in ps], dtype=np.int32),
        "tol": np.array([p["tol"] for p in ps]),
    }, ps

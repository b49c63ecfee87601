"""The SMO solvers (csrc/runtime/svm_cpu.cpp, csrc/kernels/svm.hip) against a step-exact
float64 numpy version of libsvm's ``Solver`` (docs/SVM_SOLVER_TESTS.md).

The reference runs on a kernel matrix that emulates the solvers' float32 arithmetic (an FMA
chain over the features in ascending order, the kernel function in float64, one cast), so
the host solver must reproduce it in every bit.  The GPU solvers are checked one SMO step at
a time from their own state (single-iteration launches), then at the end of the run through
the box, the equality constraint, the recomputed gradient, the KKT gap and the objective,
and the split solver against the one-workgroup solver bit for bit."""
import functools
import json
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.models import svm
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.models.svm import KLIN, KPOLY, KRBF, KSIG, PROB_DTYPE

TAU = 1e-12
INF = 1e300          # the solvers' "no candidate" value
NEAR_TIE = 1e-9      # a step whose best and runner-up candidates are closer than this is not compared
MAX_SKIP = 0.05      # ... and at most this fraction of a problem's steps may be such near-ties
STEP_LAUNCHES = 200  # single-iteration launches at the start of a stepped run
RESUME_CHUNK = 37    # then one resumed launch of this many iterations, then the rest
U53 = 2.0 ** -52
_exp = np.frompyfunc(math.exp, 1, 1)     # libm's exp / tanh: what the host solver calls
_tanh = np.frompyfunc(math.tanh, 1, 1)


# ======================================================================================
# reference: emulated float32 kernel values, one SMO step, the solve loop
# ======================================================================================
def _k32(A, B, kernel, gamma, coef0, degree):
    """Kernel values of the rows A[..., :] and B[..., :] (float32, broadcast over the leading
    axes) with the solvers' arithmetic: acc <- fl32(acc + t * t) (RBF, t = fl32(a - b)) or
    fl32(acc + a * b) per feature in ascending order -- float32 products are exact in
    float64, so the float64 sum rounded to float32 is the fused multiply-add -- then the
    kernel function in float64, cast to float32.  Returned as float64 (exact)."""
    A = np.asarray(A, dtype=np.float32)
    B = np.asarray(B, dtype=np.float32)
    acc = np.zeros(np.broadcast(A[..., 0], B[..., 0]).shape, dtype=np.float32)
    for f in range(A.shape[-1]):
        a, b = A[..., f], B[..., f]
        if kernel == KRBF:
            t = (a - b).astype(np.float64)
            acc = (acc.astype(np.float64) + t * t).astype(np.float32)
        else:
            acc = (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    acc = acc.astype(np.float64)
    if kernel == KRBF:
        out = _exp(-gamma * acc).astype(np.float64)
    elif kernel == KPOLY:
        b = gamma * acc + coef0
        out = np.ones_like(b)
        for _ in range(int(degree)):
            out = out * b
    elif kernel == KSIG:
        out = _tanh(gamma * acc + coef0).astype(np.float64)
    else:
        out = acc
    return out.astype(np.float32).astype(np.float64)


def k32(X, kernel, gamma, coef0, degree):
    """The emulated float32 kernel matrix of the rows of X, as float64 [n, n]."""
    X = np.asarray(X, dtype=np.float32)
    return _k32(X[:, None, :], X[None, :, :], kernel, gamma, coef0, degree)


class KernelQ:
    """Q = (y y^T) * K32 of one dual problem, columns computed on demand: ``col(r)`` is the
    kernel column of rowset row r (float64 holding float32 values), ``qd`` the diagonal the
    solvers are given (float32 values), variable t uses row t mod nr."""

    def __init__(self, X, kernel, gamma, coef0, degree, qd):
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.nr = self.X.shape[0]
        self.kernel, self.gamma, self.coef0, self.degree = kernel, gamma, coef0, degree
        self.qd = np.asarray(qd, dtype=np.float32).astype(np.float64)
        self.kmax = float(np.abs(self.qd).max())
        self._cols = {}
        self._K = None

    def precompute(self):
        if self._K is None:
            self._K = k32(self.X, self.kernel, self.gamma, self.coef0, self.degree)
            self.kmax = max(self.kmax, float(np.abs(self._K).max()))
        return self._K

    def col(self, r):
        r = int(r)
        if self._K is not None:
            return self._K[r]
        c = self._cols.get(r)
        if c is None:
            c = _k32(self.X[r][None, :], self.X, self.kernel, self.gamma, self.coef0, self.degree)
            self._cols[r] = c
            self.kmax = max(self.kmax, float(np.abs(c).max()))
        return c

    def times(self, coef):
        """K32 @ coef for a per-row coefficient vector (only its non-zero columns are needed)."""
        out = np.zeros(self.nr)
        for r in np.nonzero(coef)[0]:
            out += self.col(r) * coef[r]
        return out


def _margin(vals, best):
    """Relative gap between the best candidate value and the runner-up; candidates exactly
    equal to the best are the index tie rule's business, not a margin problem."""
    others = vals[vals != best]
    if others.size == 0:
        return math.inf
    ru = others[np.argmin(np.abs(others - best))]
    return abs(best - ru) / max(abs(best), abs(ru), 1e-300)


def _last(mask_vals, value):
    return int(np.nonzero(mask_vals == value)[0][-1])


def smo_step(Q, p, y, C, alpha, G, eps):
    """One iteration of libsvm's Solver on the state (alpha, G): WSS3 working-set selection
    (the later index wins exact ties), the analytic two-variable update with box clipping,
    G += Q_i d_i + Q_j d_j.  ``p`` (the linear term) is part of the problem but not of a
    step: G carries it.  Returns (i, j, alpha', G', done, margin_i, margin_j); done = the
    stopping rule fired and nothing changed."""
    L, nr = len(y), Q.nr
    rows = np.arange(L) % nr
    up = np.where(y > 0, alpha < C, alpha > 0)
    if not up.any():
        return -1, -1, alpha, G, True, math.inf, math.inf
    v = np.where(up, -y * G, -np.inf)
    Gmax = v.max()
    i = _last(v, Gmax)
    margin_i = _margin(v[up], Gmax)
    yi, ri = y[i], rows[i]
    Ki = Q.col(ri)
    low = np.where(y > 0, alpha > 0, alpha < C)
    yG = y * G
    Gmax2 = yG[low].max() if low.any() else -INF
    gd = Gmax + yG
    cand = low & (gd > 0)
    qc = (Q.qd[ri] + Q.qd[rows]) - 2.0 * Ki[rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        od = np.where(qc > 0, -(gd * gd) / qc, -(gd * gd) / TAU)
    od = np.where(cand, od, np.inf)
    if Gmax + Gmax2 < eps or not cand.any():
        return i, -1, alpha, G, True, margin_i, math.inf
    odmin = od.min()
    j = _last(od, odmin)
    margin_j = _margin(od[cand], odmin)
    yj, rj = y[j], rows[j]
    Kj = Q.col(rj)
    Ci, Cj = C[i], C[j]
    Qij = yi * yj * Ki[rj]
    QDi, QDj = Q.qd[ri], Q.qd[rj]
    oai, oaj = alpha[i], alpha[j]
    ai, aj = oai, oaj
    if yi != yj:
        qq = QDi + QDj + 2.0 * Qij
        if qq <= 0:
            qq = TAU
        delta = (-G[i] - G[j]) / qq
        diff = ai - aj
        ai += delta
        aj += delta
        if diff > 0:
            if aj < 0:
                aj, ai = 0.0, diff
        elif ai < 0:
            ai, aj = 0.0, -diff
        if diff > Ci - Cj:
            if ai > Ci:
                ai, aj = Ci, Ci - diff
        elif aj > Cj:
            aj, ai = Cj, Cj + diff
    else:
        qq = QDi + QDj - 2.0 * Qij
        if qq <= 0:
            qq = TAU
        delta = (G[i] - G[j]) / qq
        sm = ai + aj
        ai -= delta
        aj += delta
        if sm > Ci:
            if ai > Ci:
                ai, aj = Ci, sm - Ci
        elif aj < 0:
            aj, ai = 0.0, sm
        if sm > Cj:
            if aj > Cj:
                aj, ai = Cj, sm - Cj
        elif ai < 0:
            ai, aj = 0.0, sm
    a2 = alpha.copy()
    a2[i], a2[j] = ai, aj          # the solvers store a[i] first, then a[j]
    dai, daj = ai - oai, aj - oaj
    G2 = G + y * ((yi * Ki[rows]) * dai + (yj * Kj[rows]) * daj)
    return i, j, a2, G2, False, margin_i, margin_j


def smo_solve(Q, p, y, C, eps, max_iter, alpha=None, G=None):
    """Iterates smo_step from alpha = 0, G = p.  Returns alpha, G, iters, status (1 optimal,
    2 iteration limit), the (i, j) sequence and the per-step margins."""
    alpha = np.zeros(len(y)) if alpha is None else alpha.copy()
    G = p.copy() if G is None else G.copy()
    it, status, seq, margins = 0, 2, [], []
    while it < max_iter:
        i, j, alpha, G, done, mi, mj = smo_step(Q, p, y, C, alpha, G, eps)
        if done:
            status = 1
            break
        seq.append((i, j))
        margins.append(min(mi, mj))
        it += 1
    return SimpleNamespace(alpha=alpha, G=G, iters=it, status=status, seq=seq, margins=np.array(margins))


# ======================================================================================
# problems
# ======================================================================================
_KID = {"linear": KLIN, "poly": KPOLY, "rbf": KRBF, "sigmoid": KSIG}


class Problem:
    """One dual problem: X [nr, d] float32, y (+-1), C, p = G0, qd, Q and the solver settings."""

    def __init__(self, X, y, C, p, kernel, gamma, coef0, degree, eps, max_iter, svr):
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.nr, self.d = self.X.shape
        self.y, self.C, self.p = y.astype(np.float64), C.astype(np.float64), p.astype(np.float64)
        self.L = len(y)
        self.kernel, self.gamma, self.coef0, self.degree = kernel, float(gamma), float(coef0), int(degree)
        self.eps, self.max_iter, self.svr = float(eps), int(max_iter), bool(svr)
        qd = _k32(self.X, self.X, kernel, self.gamma, self.coef0, self.degree)   # the diagonal of k32
        self.Q = KernelQ(self.X, kernel, self.gamma, self.coef0, self.degree, qd)
        if self.nr <= 2100:
            self.Q.precompute()
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = smo_solve(self.Q, self.p, self.y, self.C, self.eps, self.max_iter)
        return self._ref

    def gradient(self, alpha):
        """G_ref = Q32 alpha + p in float64."""
        coef = np.zeros(self.nr)
        np.add.at(coef, np.arange(self.L) % self.nr, self.y * alpha)
        return self.y * self.Q.times(coef)[np.arange(self.L) % self.nr] + self.p

    def objective(self, alpha, G_ref):
        return 0.5 * float(alpha @ (G_ref + self.p))

    def kkt(self, alpha, G_ref):
        """(m, M): max over I_up of -y G and min over I_low of -y G."""
        y, C = self.y, self.C
        up = np.where(y > 0, alpha < C, alpha > 0)
        low = np.where(y > 0, alpha > 0, alpha < C)
        v = -y * G_ref
        return (v[up].max() if up.any() else -math.inf), (v[low].min() if low.any() else math.inf)

    def duality_gap(self, alpha, G_ref):
        """D(alpha) >= f(alpha) - f*: by convexity f(b) >= f(a) + G^T (b - a), and for a
        feasible b, y^T (b - a) = 0, so f* >= f(a) + min over the box of (G + rho y)^T (b - a)
        for any rho; rho = (m + M) / 2."""
        m, M = self.kkt(alpha, G_ref)
        rho = 0.5 * (m + M) if math.isfinite(m) and math.isfinite(M) else (m if math.isfinite(m) else M)
        gt = G_ref + rho * self.y
        return float(np.sum(np.maximum(gt, 0) * alpha + np.maximum(-gt, 0) * (self.C - alpha)))


@functools.lru_cache(maxsize=None)
def make_problem(nr, d, kernel, svr=False, C=1.0, eps=1e-3, max_iter=10_000_000, seed=0):
    """y = sign(x0 + 0.5 x1^2 + 0.5 noise - 0.3) on RandomState(seed).randn inputs, C+ = 2 C-
    (per-variable C, as class weights give); SVR: that score as the target, epsilon = 0.1."""
    rng = np.random.RandomState(seed)
    X = rng.randn(nr, d).astype(np.float32)
    noise = rng.randn(nr)
    x1 = X[:, 1].astype(np.float64) if d > 1 else np.zeros(nr)
    s = X[:, 0].astype(np.float64) + 0.5 * x1 ** 2 + 0.5 * noise - 0.3
    gamma, coef0, degree = 1.0 / d, (1.0 if kernel == "poly" else 0.0), 3
    if svr:
        t = s.astype(np.float32).astype(np.float64)
        y = np.concatenate([np.ones(nr), -np.ones(nr)])
        p = np.concatenate([0.1 - t, 0.1 + t])
        Cv = np.full(2 * nr, C)
    else:
        y = np.where(s >= 0, 1.0, -1.0)
        p = -np.ones(nr)
        Cv = np.where(y > 0, 2.0 * C, C)
    return Problem(X, y, Cv, p, _KID[kernel], gamma, coef0, degree, eps, max_iter, svr)


# the problems of the host comparison, as (nr, d, kernel, svr)
SIX = [(300, 5, "rbf", False), (2049, 9, "rbf", False), (700, 33, "poly", False), (515, 7, "linear", False),
       (600, 6, "rbf", True), (257, 3, "sigmoid", False)]
_PAD = 37            # guard elements in front of and behind every per-variable / per-row array


class Batch:
    """The solver inputs of several problems with one feature count (narrower problems get
    zero features: they add exact zeros to every accumulator): PROB_DTYPE records and Xrs, y,
    C, qd, alpha, G with non-zero offsets and guard values at both ends."""

    def __init__(self, problems, max_iter=None):
        self.problems = problems
        self.d = max(pr.d for pr in problems)
        xs, ys, Cs, qds, Gs = [np.full(_PAD, 3.0, np.float32)], [np.zeros(_PAD, np.float32)], [np.full(_PAD, 5.0)], \
            [np.full(_PAD, 2.0, np.float32)], [np.full(_PAD, 9.0)]
        recs, self.views = [], []
        xoff = voff = roff = _PAD
        koff = 0
        for pr in problems:
            Xp = np.zeros((pr.nr, self.d), np.float32)
            Xp[:, :pr.d] = pr.X
            xs.append(Xp.T.reshape(-1))            # feature-major
            ys.append(pr.y.astype(np.float32)); Cs.append(pr.C); Gs.append(pr.p)
            qds.append(pr.Q.qd.astype(np.float32))
            mi = pr.max_iter if max_iter is None else max_iter
            recs.append((xoff, roff, pr.nr, pr.L, voff, koff, pr.kernel, pr.degree, pr.gamma, pr.coef0, pr.eps, mi,
                         0, 0, int(pr.svr), 0, 0))
            self.views.append(slice(voff, voff + pr.L))
            xoff += pr.nr * self.d; voff += pr.L; roff += pr.nr; koff += 2 * pr.nr
        for lst, v in ((xs, 3.0), (ys, 0.0), (Cs, 5.0), (qds, 2.0), (Gs, 9.0)):
            lst.append(np.full(_PAD, v, lst[0].dtype))
        self.P = np.array(recs, dtype=PROB_DTYPE)
        self.Xrs, self.y, self.C = np.concatenate(xs), np.concatenate(ys), np.concatenate(Cs)
        self.qd, self.G0 = np.concatenate(qds), np.concatenate(Gs)
        self.alpha0 = np.zeros_like(self.G0)
        self.alpha0[:_PAD] = self.alpha0[-_PAD:] = 7.0
        self.kbuf_len = koff
        self.guard = np.ones(len(self.G0), bool)
        for v in self.views:
            self.guard[v] = False


def solve(batch, device, hook=None):
    """Runs SVMFamily._solve on the batch (a stub ``data``: is_gpu, device, d).  ``hook`` gets
    the alpha / G tensors before the call.  Returns P, alpha, G (numpy) and the solve stats."""
    fam = family_of("SVC")
    dev = torch.device(device)
    data = SimpleNamespace(is_gpu=dev.type == "cuda", device=dev, d=batch.d)
    t = {k: torch.from_numpy(getattr(batch, k).copy()).to(dev) for k in ("Xrs", "y", "C", "qd", "alpha0", "G0")}
    P = batch.P.copy()
    if hook is not None:
        hook(t["alpha0"], t["G0"])
    fam._solve(data, P, t["Xrs"], t["y"], t["C"], t["qd"], t["alpha0"], t["G0"], batch.kbuf_len)
    alpha, G = t["alpha0"].cpu().numpy(), t["G0"].cpu().numpy()
    # nothing outside the problems' own variables was written
    assert np.array_equal(alpha[batch.guard], batch.alpha0[batch.guard])
    assert np.array_equal(G[batch.guard], batch.G0[batch.guard])
    return P, alpha, G, dict(fam.last_solve_stats)


# ======================================================================================
# CPU: the host solver reproduces the reference in every bit
# ======================================================================================
def _assert_host_equals_reference(batch):
    P, alpha, G, stats = solve(batch, "cpu")
    assert stats["solver"] == "host"
    for k, (pr, v) in enumerate(zip(batch.problems, batch.views)):
        mi = int(batch.P["max_iter"][k])
        ref = pr.ref if mi == pr.max_iter else smo_solve(pr.Q, pr.p, pr.y, pr.C, pr.eps, mi)
        assert (int(P["iters"][k]), int(P["status"][k])) == (ref.iters, ref.status), (k, P[k], ref.iters, ref.status)
        assert np.array_equal(alpha[v], ref.alpha), k
        assert np.array_equal(G[v], ref.G), k
    return P


@pytest.mark.parametrize("nr,d,kernel,svr", SIX)
def test_host_solver_equals_reference(nr, d, kernel, svr):
    pr = make_problem(nr, d, kernel, svr)
    P = _assert_host_equals_reference(Batch([pr]))
    assert int(P["status"][0]) == 1 and int(P["iters"][0]) > 20
    # the reference's own near-ties: the GPU step checks may skip at most MAX_SKIP of the steps
    assert np.mean(pr.ref.margins[:STEP_LAUNCHES] < NEAR_TIE) <= MAX_SKIP


def test_host_solver_equals_reference_mixed_batch():
    _assert_host_equals_reference(Batch([make_problem(257, 3, "sigmoid"), make_problem(600, 6, "rbf", True),
                                         make_problem(515, 7, "linear")]))


def test_host_solver_iteration_limit():
    P = _assert_host_equals_reference(Batch([make_problem(300, 5, "rbf")], max_iter=50))
    assert (int(P["iters"][0]), int(P["status"][0])) == (50, 2)


def test_host_solver_one_feature():
    _assert_host_equals_reference(Batch([make_problem(130, 1, "rbf")]))


def test_k32_is_the_host_solver_kernel_column():
    """One SMO iteration from alpha = 0 moves G by y (y_i K_i d_i + y_j K_j d_j): the host
    solver's kernel columns are k32's, for every kernel (the step itself is compared above)."""
    for kernel in ("rbf", "poly", "linear", "sigmoid"):
        pr = make_problem(130, 17, kernel)
        P, alpha, G, _ = solve(Batch([pr], max_iter=1), "cpu")
        i, j, a2, G2, done, _, _ = smo_step(pr.Q, pr.p, pr.y, pr.C, np.zeros(pr.L), pr.p, pr.eps)
        assert not done and np.array_equal(G[_PAD:-_PAD], G2) and np.array_equal(alpha[_PAD:-_PAD], a2)
        K = k32(pr.X, pr.kernel, pr.gamma, pr.coef0, pr.degree)
        assert np.array_equal(K, K.T) and np.array_equal(np.diag(K), pr.Q.qd)


# ---- the arrays SVMFamily.run builds ---------------------------------------------------
def _captured_run(model, X, y, clf, params, monkeypatch):
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.search.cv import make_split_roles

    dd = DeviceData(X, y, clf, "cpu")
    roles, names = make_split_roles(np.asarray(y), 2, clf, holdout=False, random_state=0)
    dd.set_splits(roles, names)
    fam = family_of(model)
    tasks = [FitTask(s, 0, s, model, fam.resolve(model, params, dd.train_counts[s], dd.d, dd.n_classes))
             for s in range(len(names))]
    got = {}
    real = fam._solve

    def capture(data, P, Xrs, yv, C, qd, alpha, G, kbuf_len):
        got.update(P=P.copy(), Xrs=Xrs.numpy().copy(), y=yv.numpy().copy(), C=C.numpy().copy(), qd=qd.numpy().copy(),
                   alpha=alpha.numpy().copy(), G=G.numpy().copy(), kbuf_len=kbuf_len)
        return real(data, P, Xrs, yv, C, qd, alpha, G, kbuf_len)

    monkeypatch.setattr(fam, "_solve", capture, raising=False)
    outs = fam.run(dd, tasks)
    assert all(o.error is None for o in outs)
    return dd, tasks, got


def _check_rows(got, k, X, rows, d):
    """Record k's feature-major block is X[rows]^T; returns its (voff, roff, L)."""
    rec = got["P"][k]
    nr = len(rows)
    assert int(rec["nrows"]) == nr
    blk = got["Xrs"][int(rec["xoff"]):int(rec["xoff"]) + nr * d].reshape(d, nr)
    assert np.array_equal(blk, X[rows].T)
    return int(rec["voff"]), int(rec["roff"]), int(rec["L"])


def test_run_builds_svc_problem_arrays(monkeypatch):
    rng = np.random.RandomState(11)
    n, d = 240, 5
    X = rng.randn(n, d).astype(np.float32)
    y = np.digitize(X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.3 * rng.randn(n), [-0.4, 0.9])   # 3 unbalanced classes
    params = {"C": 0.7, "kernel": "poly", "degree": 3, "gamma": 0.3, "coef0": 1.0, "class_weight": "balanced"}
    dd, tasks, got = _captured_run("SVC", X, y, True, params, monkeypatch)
    pairs = [(0, 1), (0, 2), (1, 2)]
    assert len(got["P"]) == len(tasks) * len(pairs)
    assert not got["alpha"].any()
    k = 0
    for t in tasks:
        tr = dd.train_rows[t.split].numpy().astype(np.int64)
        cnt = np.bincount(y[tr], minlength=3).astype(np.float64)
        w = len(tr) / (3.0 * cnt)                                   # sklearn's 'balanced'
        for a, b in pairs:
            rows = tr[(y[tr] == a) | (y[tr] == b)]
            v0, r0, L = _check_rows(got, k, X, rows, d)
            assert L == len(rows)
            cls = y[rows]
            assert np.array_equal(got["y"][v0:v0 + L], np.where(cls == a, 1.0, -1.0).astype(np.float32))
            # C * n / (3 n_c): a quotient and two products, each within half an ulp however grouped
            np.testing.assert_allclose(got["C"][v0:v0 + L], 0.7 * np.where(cls == a, w[a], w[b]), rtol=2.0 ** -51,
                                       atol=0)
            assert np.array_equal(got["G"][v0:v0 + L], -np.ones(L))
            n2 = (X[rows].astype(np.float64) ** 2).sum(1)
            assert np.array_equal(got["qd"][r0:r0 + L], ((0.3 * n2 + 1.0) ** 3).astype(np.float32))
            # ... which is k32's diagonal up to the float32 FMA chain's rounding of the norm
            # ((d + 1) half-ulps of positive terms, cubed) and the final cast
            diag = _k32(X[rows], X[rows], KPOLY, 0.3, 1.0, 3)
            np.testing.assert_allclose(got["qd"][r0:r0 + L], diag, rtol=(3 * (d + 1) + 2) * 2.0 ** -24, atol=0)
            rec = got["P"][k]
            assert (int(rec["kernel"]), int(rec["degree"]), float(rec["gamma"]), float(rec["coef0"]), float(rec["eps"]),
                    int(rec["svr"])) == (KPOLY, 3, 0.3, 1.0, 1e-3, 0)
            k += 1
    assert got["kbuf_len"] == 2 * int(got["P"]["nrows"].sum())


def test_run_builds_svr_problem_arrays(monkeypatch):
    rng = np.random.RandomState(12)
    n, d = 150, 4
    X = rng.randn(n, d).astype(np.float32)
    y = (np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rng.randn(n)).astype(np.float32)
    dd, tasks, got = _captured_run("SVR", X, y, False, {"C": 1.5, "epsilon": 0.2, "gamma": 0.25}, monkeypatch)
    assert len(got["P"]) == len(tasks)
    for k, t in enumerate(tasks):
        rows = dd.train_rows[t.split].numpy().astype(np.int64)
        nr = len(rows)
        v0, r0, L = _check_rows(got, k, X, rows, d)
        assert L == 2 * nr and int(got["P"][k]["svr"]) == 1
        yv = y[rows].astype(np.float64)
        assert np.array_equal(got["y"][v0:v0 + L], np.concatenate([np.ones(nr), -np.ones(nr)]).astype(np.float32))
        assert np.array_equal(got["C"][v0:v0 + L], np.full(L, 1.5))
        assert np.array_equal(got["G"][v0:v0 + L], np.concatenate([0.2 - yv, 0.2 + yv]))
        assert np.array_equal(got["qd"][r0:r0 + nr], np.ones(nr, np.float32))
        assert np.array_equal(got["qd"][r0:r0 + nr], _k32(X[rows], X[rows], KRBF, 0.25, 0.0, 3))


# ======================================================================================
# GPU: every single step from the GPU's own state, then the end state
# ======================================================================================
class Recorder:
    """Wraps dml_svm_smo / dml_svm_smo_split: synchronises and snapshots alpha and G after
    every launch, and sets the next launch's chunk (1 x STEP_LAUNCHES, RESUME_CHUNK, the rest;
    or ``fixed_chunk`` throughout)."""

    def __init__(self, monkeypatch, lib, fixed_chunk=None):
        self.mp, self.fixed = monkeypatch, fixed_chunk
        self.snaps, self.launches = [], []
        self.alpha = self.G = None
        for name, chunk_arg in (("dml_svm_smo", 10), ("dml_svm_smo_split", 15)):
            monkeypatch.setattr(lib, name, self._wrap(getattr(lib, name), name, chunk_arg), raising=False)
        self._set_chunk()

    def _set_chunk(self):
        n = len(self.launches)
        if self.fixed is not None:
            c = self.fixed
        else:
            c = 1 if n < STEP_LAUNCHES else RESUME_CHUNK if n == STEP_LAUNCHES else 50_000
        self.mp.setattr(svm, "CHUNK_ITERS", c)
        self.mp.setattr(svm, "SPLIT_CHUNK_ITERS", c)

    def hook(self, alpha, G):
        self.alpha, self.G = alpha, G
        self.snaps.append((alpha.cpu().numpy(), G.cpu().numpy()))

    def _wrap(self, fn, name, chunk_arg):
        def launch(*args):
            rc = fn(*args)
            torch.cuda.synchronize()
            self.snaps.append((self.alpha.cpu().numpy(), self.G.cpu().numpy()))
            self.launches.append({"fn": name, "chunk": int(args[chunk_arg]),
                                  "B": int(args[4]) if name.endswith("split") else 1,
                                  "wide": int(args[17]) if name.endswith("split") else 0})
            self._set_chunk()
            return rc
        return launch


def check_steps(pr, view, rec):
    """Applies smo_step to the GPU's state before every single-iteration launch and compares
    with its state after it.  Returns (steps, skipped)."""
    maxC = float(pr.C.max())
    it = steps = skipped = 0
    finished = False
    for n, launch in enumerate(rec.launches):
        if launch["chunk"] != 1:
            break
        a0, g0 = rec.snaps[n][0][view], rec.snaps[n][1][view]
        a1, g1 = rec.snaps[n + 1][0][view], rec.snaps[n + 1][1][view]
        done = finished or it >= pr.max_iter
        if not done:
            i, j, ar, gr, done, mi, mj = smo_step(pr.Q, pr.p, pr.y, pr.C, a0, g0, pr.eps)
        if done:
            finished = True
            assert np.array_equal(a1, a0) and np.array_equal(g1, g0), f"launch {n}: a finished problem moved"
            continue
        it += 1
        steps += 1
        if min(mi, mj) < NEAR_TIE:
            skipped += 1
            continue
        changed = set(np.nonzero(a1 != a0)[0].tolist())
        assert changed == set(np.nonzero(ar != a0)[0].tolist()) and changed <= {i, j}, \
            f"launch {n}: variables {sorted(changed)} moved, the reference moves ({i}, {j})"
        ea = float(np.abs(a1 - ar).max())
        assert ea <= 4 * U53 * maxC, f"launch {n} (i={i}, j={j}): alpha off by {ea:.3e}"
        gtol = 8 * U53 * max(1.0, float(np.abs(g0).max()), float(np.abs(gr).max()), pr.Q.kmax * maxC)
        eg = np.abs(g1 - gr)
        assert float(eg.max()) <= gtol, \
            f"launch {n} (i={i}, j={j}): G[{int(eg.argmax())}] off by {float(eg.max()):.3e} > {gtol:.3e}"
    assert skipped <= MAX_SKIP * max(steps, 1), (steps, skipped)
    return steps, skipped


def check_end(pr, max_iter, alpha, G, iters, status):
    """Box, equality, gradient, KKT gap and objective of a finished run.  Returns whether the
    run ended bit-identical to the reference."""
    ref = pr.ref if max_iter == pr.max_iter else smo_solve(pr.Q, pr.p, pr.y, pr.C, pr.eps, max_iter)
    maxC = float(pr.C.max())
    assert np.all(alpha >= 0) and np.all(alpha <= pr.C)
    assert abs(float(pr.y @ alpha)) <= iters * 2.0 ** -50 * maxC
    G_ref = pr.gradient(alpha)
    gtol = iters * 2.0 ** -50 * max(1.0, float(np.abs(G).max())) + 2 * 2.0 ** -24 * pr.Q.kmax * maxC
    eg = float(np.abs(G - G_ref).max())
    assert eg <= gtol, f"maintained gradient off by {eg:.3e} > {gtol:.3e}"
    m, M = pr.kkt(alpha, G_ref)
    if iters >= max_iter:
        assert (iters, status) == (max_iter, 2)
    else:
        assert status == 1
        assert m - M <= pr.eps + 2 * gtol, f"KKT gap {m - M:.3e}"
    f_gpu = pr.objective(alpha, G_ref)
    Gr = pr.gradient(ref.alpha)
    f_ref = pr.objective(ref.alpha, Gr)
    bound = max(pr.duality_gap(alpha, G_ref), pr.duality_gap(ref.alpha, Gr))
    assert abs(f_gpu - f_ref) <= bound, (f_gpu, f_ref, bound)
    return bool(iters == ref.iters and np.array_equal(alpha, ref.alpha) and np.array_equal(G, ref.G))


def _report(case, t0, steps, skipped, identical):
    """One line per case (pytest -s shows it); appended to $DML_SVM_TEST_REPORT when set."""
    line = {"case": case, "steps": steps, "skipped": skipped, "bit_identical_to_reference": identical,
            "seconds": round(time.perf_counter() - t0, 2)}
    print("svm-solver-case", json.dumps(line))
    if os.environ.get("DML_SVM_TEST_REPORT"):
        with open(os.environ["DML_SVM_TEST_REPORT"], "a") as f:
            f.write(json.dumps(line) + "\n")


def run_case(case, monkeypatch, problems, split, wide=1, min_rows=None, slots=None, max_iter=None, fixed_chunk=None,
             expect=None):
    """The stepped run of a batch through SVMFamily._solve with the step and end checks; for a
    split run also the one-workgroup solver on the same batch, which must agree in every bit.
    ``expect(stats, launches)`` asserts that the intended path ran."""
    from cs230_distributed_machine_learning_amd.utils import native

    t0 = time.perf_counter()
    lib = native.hip_lib()
    monkeypatch.setenv("DML_SVM_SPLIT", "1" if split else "0")
    monkeypatch.setenv("DML_SVM_WIDE", str(wide))
    monkeypatch.delenv("DML_SVM_PROFILE", raising=False)
    if slots is None:
        monkeypatch.delenv("DML_SVM_CACHE_SLOTS", raising=False)
    else:
        monkeypatch.setenv("DML_SVM_CACHE_SLOTS", str(slots))
    if min_rows is not None:
        monkeypatch.setattr(svm, "MIN_ROWS_PER_WG", min_rows)
    batch = Batch(problems, max_iter=max_iter)
    rec = Recorder(monkeypatch, lib, fixed_chunk=fixed_chunk)
    P, alpha, G, stats = solve(batch, "cuda:0", rec.hook)
    assert stats["solver"] == ("split" if split else "one workgroup per problem"), stats
    assert all(l["fn"] == ("dml_svm_smo_split" if split else "dml_svm_smo") for l in rec.launches)
    if expect is not None:
        expect(stats, rec.launches)
    steps = skipped = 0
    identical = True
    for k, (pr, v) in enumerate(zip(batch.problems, batch.views)):
        s, sk = check_steps(pr, v, rec)
        steps, skipped = steps + s, skipped + sk
        identical &= check_end(pr, int(batch.P["max_iter"][k]), alpha[v], G[v], int(P["iters"][k]), int(P["status"][k]))
    if split:
        monkeypatch.setenv("DML_SVM_SPLIT", "0")
        monkeypatch.setattr(svm, "CHUNK_ITERS", 20000)
        P1, alpha1, G1, stats1 = solve(batch, "cuda:0", rec.hook)
        assert stats1["solver"] == "one workgroup per problem"
        assert np.array_equal(P["iters"], P1["iters"]) and np.array_equal(P["status"], P1["status"])
        assert np.array_equal(alpha, alpha1) and np.array_equal(G, G1)
    _report(case, t0, steps, skipped, identical)
    return stats, rec


@pytest.mark.gpu
@pytest.mark.parametrize("nr,d,kernel,svr", SIX)
def test_gpu_one_workgroup_solver_steps(nr, d, kernel, svr, monkeypatch):
    run_case(f"k_smo {nr}x{d} {kernel}{' svr' if svr else ''}", monkeypatch, [make_problem(nr, d, kernel, svr)],
             split=False)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
def test_gpu_split_solver_steps_batch_of_six(wide, monkeypatch):
    """Non-zero offsets, all four kernels, SVR and weighted C at B = 21 down to 4 (the batch
    re-splits as its larger problems finish): slices of 12 to 100 rows."""
    def expect(stats, launches):
        assert stats["workgroups_per_launch"][0] == 21
        assert (stats["wide_launches"] > 0) == bool(wide)
        assert stats["cache_slots"] == 2049

    run_case(f"split batch of six, wide={wide}", monkeypatch, [make_problem(*s) for s in SIX], split=True, wide=wide,
             min_rows=64, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
def test_gpu_split_solver_steps_slices_below_a_wave(wide, monkeypatch):
    def expect(stats, launches):
        assert stats["workgroups_per_launch"] == [21] * stats["launches"]      # kMaxB; slices of 24 or 25 rows
        assert stats["wide_launches"] == wide * stats["launches"]

    run_case(f"split 515 rows, B=21, wide={wide}", monkeypatch, [make_problem(515, 7, "linear")], split=True, wide=wide,
             min_rows=24, expect=expect)


@pytest.mark.gpu
@pytest.mark.parametrize("nr,min_rows,B,wide_runs", [(2048, 4096, 1, True), (2049, 4096, 1, False),
                                                     (1100, 500, 2, True)])
def test_gpu_split_solver_steps_register_state(nr, min_rows, B, wide_runs, monkeypatch):
    """The wide variant keeps a slice of up to 2048 variables in registers: exactly full (2048
    at B = 1), one past it (2049: the host must take the narrow variant) and two slices of 550
    (tail lanes clamped)."""
    def expect(stats, launches):
        assert stats["workgroups_per_launch"] == [B] * stats["launches"]
        assert stats["wide_launches"] == (stats["launches"] if wide_runs else 0)

    run_case(f"split {nr} rows, B={B}, wide=1", monkeypatch, [make_problem(nr, 9, "rbf")], split=True, wide=1,
             min_rows=min_rows, expect=expect)


FEATURE_CASES = [(130, 1, "rbf"), (130, 15, "poly"), (130, 16, "rbf"), (130, 17, "sigmoid"), (70, 2048, "rbf"),
                 (70, 2050, "poly")]


@pytest.mark.parametrize("nr,d,kernel", FEATURE_CASES + [(2048, 9, "rbf"), (1100, 9, "rbf")])
def test_gpu_case_inputs_have_few_near_ties(nr, d, kernel):
    """The inputs of the GPU cases that are not among the six: the reference converges on
    them and at most MAX_SKIP of its first steps are near-ties."""
    ref = make_problem(nr, d, kernel).ref
    assert ref.status == 1 and ref.iters > 50
    assert np.mean(ref.margins[:STEP_LAUNCHES] < NEAR_TIE) <= MAX_SKIP


@pytest.mark.gpu
@pytest.mark.parametrize("nr,d,kernel", FEATURE_CASES)
@pytest.mark.parametrize("split", [True, False])
def test_gpu_solver_steps_feature_counts(nr, d, kernel, split, monkeypatch):
    """d below, at and past the 16-feature column block; d at the LDS staging limit of the
    query row (2048) and past it (the query row is read from memory)."""
    def expect(stats, launches):
        if split:
            assert stats["workgroups_per_problem"] == nr // 32

    run_case(f"{'split' if split else 'k_smo'} {nr}x{d} {kernel}", monkeypatch, [make_problem(nr, d, kernel)],
             split=split, wide=0, min_rows=32, expect=expect)


@functools.lru_cache(maxsize=None)
def cache_problem():
    return make_problem(700, 33, "poly", False, 4.0)


def test_cache_case_touches_more_rows_than_slots():
    """The cache cases evict: the reference's working sets visit more distinct rows than the
    largest forced cache (300 slots), and have almost no near-ties."""
    ref = cache_problem().ref
    assert len({r for ij in ref.seq for r in ij}) > 300 and ref.status == 1
    assert np.mean(ref.margins[:STEP_LAUNCHES] < NEAR_TIE) <= MAX_SKIP


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [2, 256, 300])
def test_gpu_split_solver_steps_cache_eviction(slots, monkeypatch):
    """2 slots: both columns evicted every step; 256: exact LRU over all slots; 300: victims
    among 256 hashed samples."""
    def expect(stats, launches):
        assert stats["cache_slots"] == slots and stats["workgroups_per_problem"] == 5

    run_case(f"split 700 rows, {slots} cache slots", monkeypatch, [cache_problem()], split=True, wide=1, min_rows=128,
             slots=slots, expect=expect)


# ---- LDS tag collisions ------------------------------------------------------------------
_TAG_N = 4096        # svm.hip kTagN


@functools.lru_cache(maxsize=None)
def tag_problem():
    """4200 rows of which only rows [0, 10) and [4096, 4106) are hard (overlapping classes
    next to the boundary; the rest lie far from it), so the working sets keep returning to
    rows r and r + 4096, which share an LDS tag."""
    rng = np.random.RandomState(3)
    nr = 4200
    hard = np.r_[0:10, 4096:4106]
    lab = np.where(rng.rand(nr) < 0.5, 1.0, -1.0)
    X = np.empty((nr, 2), np.float32)
    X[:, 0] = lab * (3.0 + np.abs(rng.randn(nr)))
    X[:, 1] = rng.randn(nr)
    X[hard, 0] = 0.4 * rng.randn(len(hard))
    return Problem(X, lab, np.where(lab > 0, 200.0, 100.0), -np.ones(nr), KRBF, 0.5, 0.0, 3, 1e-3, 300, False)


def _tag_collisions(seq, boundaries):
    """Direct-mapped tag model: lookups of row i then row j per iteration, the tags cleared
    at every launch boundary; counts lookups that find the slot holding the other row."""
    tag, n = {}, 0
    for it, ij in enumerate(seq):
        if it in boundaries:
            tag = {}
        for r in ij:
            h = r & (_TAG_N - 1)
            if tag.get(h, r) != r:
                assert abs(tag[h] - r) == _TAG_N
                n += 1
            tag[h] = r
    return n


def test_tag_case_collides():
    ref = tag_problem().ref
    assert (ref.iters, ref.status) == (300, 2)
    # the stepped run's launches: iterations [0, 200) one each, [200, 237), [237, 300)
    assert _tag_collisions(ref.seq, set(range(STEP_LAUNCHES + 1)) | {STEP_LAUNCHES + RESUME_CHUNK}) >= 10
    assert np.mean(ref.margins[:STEP_LAUNCHES] < NEAR_TIE) <= MAX_SKIP


@pytest.mark.gpu
def test_gpu_split_solver_steps_iteration_limit_and_tag_collisions(monkeypatch):
    def expect(stats, launches):
        assert stats["workgroups_per_problem"] == 4 and stats["cache_slots"] == 4200
        assert [l["chunk"] for l in launches] == [1] * STEP_LAUNCHES + [RESUME_CHUNK, 50_000]

    stats, rec = run_case("split 4200 rows, max_iter=300", monkeypatch, [tag_problem()], split=True, wide=0,
                          expect=expect)
    assert stats["iterations_max"] == 300


# ---- replica copy when B changes between launches ---------------------------------------
def _shrink_problems():
    return [make_problem(600, 6, "rbf", False, 0.1), make_problem(200, 6, "rbf", False, 100.0, 1e-3, 10_000_000, 1)]


def test_shrink_case_ends_the_wide_problem_first():
    easy, hard = (pr.ref for pr in _shrink_problems())
    assert easy.status == hard.status == 1 and easy.iters > 50 and hard.iters > easy.iters + 100


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
def test_gpu_split_solver_replica_copy_when_b_shrinks(wide, monkeypatch):
    """600 easy rows (C = 0.1) and 200 hard ones (C = 100) in chunks of 25 iterations: B = 6
    until the first problem ends, then 2 -- workgroup 1 continues on a copy of replica 0."""
    def expect(stats, launches):
        hist = stats["workgroups_per_launch"]
        assert hist[0] == 6 and hist[-1] == 2 and sorted(hist, reverse=True) == hist, hist
        assert hist.count(2) >= 2

    run_case(f"split 600 + 200 rows, B 6 -> 2, wide={wide}", monkeypatch, _shrink_problems(), split=True, wide=wide, min_rows=100, fixed_chunk=25, expect=expect)


def _grow_problems():
    """30 problems of 200 rows with C from 0.05 to 20: the easy ones end within a few chunks."""
    Cs = np.round(0.05 * 400.0 ** (np.arange(30) / 29.0), 4)
    return [make_problem(200, 6, "rbf", False, float(C), 1e-3, 10_000_000, k) for k, C in enumerate(Cs)]


def test_grow_case_problems_end_at_different_times():
    iters = sorted(pr.ref.iters for pr in _grow_problems())
    assert iters[14] + 50 < iters[-10] and iters[-10] + 50 < iters[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [0, 1])
def test_gpu_split_solver_replica_copy_when_b_grows(wide, monkeypatch):
    """30 problems share the resident workgroups, so B starts below kMaxB and grows as
    problems end: the new workgroups start from copies of replica 0 -- with an empty map
    they would choose other cache slots than their peers for the same row."""
    def expect(stats, launches):
        hist = stats["workgroups_per_launch"]
        assert sorted(hist) == hist and 1 < hist[0] < hist[-1], hist

    run_case(f"split 30 x 200 rows, B grows, wide={wide}", monkeypatch, _grow_problems(), split=True, wide=wide,
             min_rows=8, fixed_chunk=25, expect=expect)

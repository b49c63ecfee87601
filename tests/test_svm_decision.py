"""The batched post-solve phase of SVC / SVR (docs/SVM_DECISION.md): the host twins of
csrc/kernels/svm_decision.hip against a plain numpy reference (float64 features, the direct
kernel formula, long-double sums), and ``DML_SVM_DECISION=1`` against the per-problem loop.
tests/test_svm_decision_gpu.py runs the same cases through the kernels."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.models import svm
from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
from cs230_distributed_machine_learning_amd.search.cv import make_split_roles
from cs230_distributed_machine_learning_amd.utils import native

KERNELS = {"linear": (svm.KLIN, 0, 0.0), "poly": (svm.KPOLY, 3, 1.0), "rbf": (svm.KRBF, 0, 0.0),
           "sigmoid": (svm.KSIG, 0, 0.0)}
SHAPES = [(1, 1, 1), (63, 3, 17), (257, 20, 16), (300, 257, 33), (1025, 7, 65)]   # (nrows, d, queries)
CASES = [(k, s, shape) for k in KERNELS for s in (0, 1) for shape in SHAPES]
BOUND = 1e-11    # |dec - ref| <= BOUND (sum_j |coef_j k_j| + |rho|): (nsv + d) 2^-53 ~ 1.4e-13 of summation
#                  error, and exp / tanh amplify their argument's error by |gamma acc| <= 40 here


def make_batch(kernel, svr, shape, seed=0):
    """Three problems of one call on a random float32 table; yG sits near 0.3, as at an optimum.
    "mixed": alphas at 0, at C and strictly inside, so rho is the free mean; a permuted opos;
    "zero": every alpha 0, so rho comes from both bound sets; half the queries (none when the shape
    has one); "all": every row a support vector."""
    nrows, d, nq = shape
    rng = np.random.RandomState(seed + 7 * nrows + d)
    code, degree, coef0 = KERNELS[kernel]
    X = rng.randn(1100, d).astype(np.float32)
    P = np.zeros(3, dtype=svm.PROB_DTYPE)
    b = SimpleNamespace(X=X, d=d, P=P, svr=svr, rows=[], Xrs=[], y=[], C=[], alpha=[], G=[], qrows=[], opos=[])
    qinfo, xoff, roff, voff, qoff = np.zeros((3, 2), np.int64), 0, 0, 0, 0
    problems = (("mixed", nrows, nq), ("zero", nrows // 2 + 2, nq // 2), ("all", min(nrows, 70), 3))
    for k, (kind, nr, qn) in enumerate(problems):
        L = 2 * nr if svr else nr
        rows = rng.choice(1100, nr, replace=False)
        if svr:
            y = np.concatenate([np.ones(nr), -np.ones(nr)])
        else:
            y = np.where(rng.rand(nr) < 0.5, 1.0, -1.0)
            y[:2] = (1.0, -1.0)[:nr]          # both classes present: the bound sets of "zero" are non-empty
        C = rng.choice([0.5, 2.0], L)
        u = rng.rand(L)
        inside = C * rng.uniform(0.1, 0.9, L)
        if kind == "mixed":
            alpha = np.where(u < 0.4, 0.0, np.where(u < 0.6, C, inside))
            alpha[0] = inside[0]              # at least one free variable
        else:
            alpha = np.zeros(L) if kind == "zero" else inside
        P[k] = (xoff, roff, nr, L, voff, 0, code, degree, 0.5 / d, coef0, 1e-3, 0, 0, 1, svr, 0, 0)
        b.rows.append(rows)
        b.Xrs.append(X[rows].T.reshape(-1))
        b.y.append(y.astype(np.float32))
        b.C.append(C)
        b.alpha.append(alpha)
        b.G.append(y * (0.3 + 0.01 * rng.randn(L)))
        b.qrows.append(rng.choice(1100, qn))
        b.opos.append(qoff + (rng.permutation(qn) if kind == "mixed" else np.arange(qn)))
        qinfo[k] = (qoff, qn)
        xoff, roff, voff, qoff = xoff + nr * d, roff + nr, voff + L, qoff + qn
    b.qinfo, b.nq_total = qinfo, qoff
    return b


def run_native(b, dev="cpu"):
    """rho_sv + decision of the batch on ``dev`` (the host twins on "cpu") -> rho, nsv, idx, coef, out."""
    data = SimpleNamespace(is_gpu=dev != "cpu", device=torch.device(dev))

    def flat(parts, dtype):   # the parts end to end, on the device
        joined = np.concatenate([np.ravel(x) for x in parts]).astype(dtype)
        return torch.from_numpy(np.ascontiguousarray(joined)).to(dev)

    def filled(n, dtype, value):   # outputs start from a value the kernels never write
        return torch.full((n,), value, dtype=dtype, device=dev)

    tiles = (b.qinfo[:, 1] + svm.DEC_QUERY_TILE - 1) // svm.DEC_QUERY_TILE
    work = np.stack([np.repeat(np.arange(3), tiles), np.concatenate([np.arange(n) for n in tiles])], 1)
    nr = int(b.P["nrows"].sum())
    pad = [np.zeros(1)]               # keeps the base pointers valid when there is no query
    buf = {"probs": flat([b.P.view(np.uint8)], np.uint8), "y": flat(b.y, np.float32), "C": flat(b.C, np.float64),
           "alpha": flat(b.alpha, np.float64), "G": flat(b.G, np.float64), "Xrs": flat(b.Xrs, np.float32),
           "X": flat([b.X], np.float32), "work": flat([work], np.int32), "qinfo": flat([b.qinfo], np.int64),
           "qrows": flat(b.qrows + pad, np.int64), "opos": flat(b.opos + pad, np.int64),
           "sv_idx": filled(nr, torch.int32, -1), "sv_coef": filled(nr, torch.float64, np.nan),
           "rho": filled(3, torch.float64, np.nan), "nsv": filled(3, torch.int32, -1),
           "out": filled(b.nq_total + 1, torch.float64, np.nan)}
    args = native.SvmDecArgs(nprob=3, d=b.d, nwork=len(work), **{k: native.ptr(v) for k, v in buf.items()})
    svm._native_call(data, "rho_sv", args)
    svm._native_call(data, "decision", args)
    return [buf[k].cpu().numpy() for k in ("rho", "nsv", "sv_idx", "sv_coef")] + [buf["out"].cpu().numpy()[:b.nq_total]]


def reference(b):
    """Per problem: (rho of ``_rho``, nonzero(coef), coef[sv], decision values, their error scale)."""
    ld, ref = np.longdouble, []
    for k, rec in enumerate(b.P):
        nr, a, y = int(rec["nrows"]), b.alpha[k], b.y[k].astype(np.float64)
        rho = svm._rho(*(torch.from_numpy(v) for v in (a, b.G[k], y, b.C[k])))
        coef = a[:nr] - a[nr:] if b.svr else a * y
        sv = np.nonzero(coef)[0]
        Q, S = b.X[b.qrows[k]].astype(ld), b.X[b.rows[k][sv]].astype(ld)
        acc = (((Q[:, None] - S[None]) ** 2) if rec["kernel"] == svm.KRBF else Q[:, None] * S[None]).sum(-1)
        g, c0 = ld(rec["gamma"]), ld(rec["coef0"])
        K = {svm.KLIN: lambda: acc, svm.KPOLY: lambda: (g * acc + c0) ** int(rec["degree"]),
             svm.KRBF: lambda: np.exp(-g * acc), svm.KSIG: lambda: np.tanh(g * acc + c0)}[int(rec["kernel"])]()
        terms = K * coef[sv].astype(ld)
        ref.append((rho, sv, coef[sv], (terms.sum(1) - ld(rho)).astype(np.float64), (np.abs(terms).sum(1) + abs(rho)).astype(np.float64)))
    return ref


def check_batch(b, got, label):
    """rho, the compacted support vectors and the decision values of ``run_native`` against ``reference``."""
    rho, nsv, idx, coef, out = got
    worst = 0.0
    for k, (r_rho, r_sv, r_coef, r_dec, scale) in enumerate(reference(b)):
        r0 = int(b.P[k]["roff"])
        assert nsv[k] == len(r_sv) and np.array_equal(idx[r0:r0 + nsv[k]], r_sv) and np.array_equal(coef[r0:r0 + nsv[k]], r_coef)
        assert abs(rho[k] - r_rho) <= 1e-14 * abs(r_rho)
        err = np.abs(out[b.opos[k]] - r_dec) / scale
        worst = max(worst, err.max(initial=0.0))
    print(f"{label}: max |dec - ref| / (sum |coef k| + |rho|) = {worst:.3e}")
    assert not np.isnan(out).any() and worst <= BOUND


@pytest.mark.parametrize("kernel,svr,shape", CASES)
def test_host_twins_against_numpy(kernel, svr, shape):
    b = make_batch(kernel, svr, shape)
    check_batch(b, run_native(b), f"{kernel} svr={svr} {shape}")


RHO_BRANCHES = {   # alpha / C per variable, y per variable -> the branch of calculate_rho
    "free": ([0.0, 0.5, 1.0, 0.25], [1, -1, 1, -1]),
    "both bounds": ([0.0, 1.0, 0.0, 1.0, 0.0], [1, 1, -1, -1, 1]),
    "upper bound only": ([1.0, 0.0, 1.0], [-1, 1, -1]),      # no lower bound: rho = -inf
    "lower bound only": ([1.0, 0.0, 1.0], [1, -1, 1]),       # no upper bound: rho = +inf
}


def rho_batch(case):
    frac, y = (np.asarray(v, np.float64) for v in RHO_BRANCHES[case])
    L = len(y)
    P = np.zeros(3, dtype=svm.PROB_DTYPE)
    P[:] = [(0, k * L, L, L, k * L, 0, svm.KLIN, 0, 1.0, 0.0, 1e-3, 0, 0, 1, 0, 0, 0) for k in range(3)]
    G = [np.random.RandomState(k).randn(L) for k in range(3)]
    z = [np.zeros(0, np.int64)] * 3
    return SimpleNamespace(X=np.ones((L, 1), np.float32), d=1, P=P, svr=0, rows=[np.arange(L)] * 3, Xrs=[np.ones(L)] * 3,
                           y=[y.astype(np.float32)] * 3, C=[np.full(L, 2.0)] * 3, alpha=[2.0 * frac] * 3, G=G, qrows=z,
                           opos=z, qinfo=np.zeros((3, 2), np.int64), nq_total=0)


def check_rho(b, rho):
    for k in range(3):
        want = svm._rho(*(torch.from_numpy(np.asarray(v, np.float64)) for v in (b.alpha[k], b.G[k], b.y[k], b.C[k])))
        free = ((b.alpha[k] > 0) & (b.alpha[k] < b.C[k])).any()
        assert abs(rho[k] - want) <= 1e-14 * abs(want) if free else rho[k] == want, (k, rho[k], want)


@pytest.mark.parametrize("case", list(RHO_BRANCHES))
def test_rho_branches_equal_rho(case):
    b = rho_batch(case)
    check_rho(b, run_native(b)[0])


# ---- the family: DML_SVM_DECISION=1 against the per-problem loop --------------------------------
def family_table(model, n):
    rng = np.random.RandomState(5)
    X = rng.randn(n, 6 if model == "SVC" else 5).astype(np.float32)
    z = X[:, 0] + 0.5 * X[:, 1] ** 2 + 0.3 * rng.randn(n)
    return X, (np.digitize(z, [-0.5, 0.8]) if model == "SVC" else z)     # SVC: 3 classes


def log_loss_scores(dev, n, monkeypatch):
    """mean neg_log_loss of the 2-C, cv=3 ``probability=True`` grid through the engine, per mode."""
    X, y = family_table("SVC", n)
    grid = [{"C": c, "probability": True, "random_state": 0} for c in (0.3, 3.0)]
    spec = JobSpec("SVC", grid, cv=3, holdout=False, keep_models="none", scoring="neg_log_loss")
    scores = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DML_SVM_DECISION", mode)
        res = run_candidates(DeviceData(X, y, True, dev), spec, range(len(grid)))
        assert all(r.ok for r in res), [r.error for r in res]
        scores[mode] = np.array([r.result["mean_cv_score"] for r in res])
    print(f"neg_log_loss {dev}: batched {scores['1']}, loop {scores['0']}, gap {np.abs(scores['1'] - scores['0']).max():.3e}")
    assert np.isfinite(scores["1"]).all()
    return np.abs(scores["1"] - scores["0"]).max()


def family_runs(dev, model, n, n_cand, monkeypatch, probability=False):
    """dec / cvdec / predictions / probabilities of ``SVMFamily.run`` per mode, and the modes' stats."""
    X, y = family_table(model, n)
    fam, got, real = family_of(model), {}, family_of(model)._probabilities
    for mode in ("1", "0"):
        monkeypatch.setenv("DML_SVM_DECISION", mode)
        dd = DeviceData(X, y, model == "SVC", dev)
        roles, names = make_split_roles(np.asarray(y), 3, model == "SVC", holdout=False, random_state=0)
        dd.set_splits(roles, names)
        params = [{"C": c, **({"probability": True, "random_state": 0} if probability else {})}
                  for c in (0.3, 3.0, 1.0, 10.0)[:n_cand]]
        tasks = [FitTask(len(names) * i + s, i, s, model, fam.resolve(model, p, dd.train_counts[s], dd.d, dd.n_classes),
                         need_proba=probability, scorer="neg_log_loss" if probability else None)
                 for i, p in enumerate(params) for s in range(len(names))]
        seen = {}

        def capture(data, tasks_, wants, pairs, rowsets, dec, cvdec, models):
            seen.update({("dec",) + k: v.double().cpu().numpy() for k, v in dec.items()})
            seen.update({("cv",) + k: v.double().cpu().numpy() for k, v in cvdec.items()})
            return real(data, tasks_, wants, pairs, rowsets, dec, cvdec, models)

        monkeypatch.setattr(fam, "_probabilities", capture, raising=False)
        outs = fam.run(dd, tasks)
        assert all(o.error is None for o in outs)
        seen.update({("pred", i): o.pred.cpu().numpy() for i, o in enumerate(outs)})
        seen.update({("proba", i): o.proba.cpu().numpy() for i, o in enumerate(outs) if o.proba is not None})
        got[mode] = (seen, dict(fam.last_decision_stats), dict(fam.last_solve_stats))
    return got


def check_family(got):
    (new, stats, solve), (old, _, _) = got["1"], got["0"]
    assert new.keys() == old.keys() and any(k[0] == "dec" for k in new)
    for k in new:   # class predictions are equal; decision values, SVR predictions and probabilities within 1e-9
        tol = 0 if new[k].dtype.kind == "i" else 1e-9
        assert np.abs(new[k].astype(np.float64) - old[k].astype(np.float64)).max(initial=0.0) <= tol, k
    assert stats["problems"] == solve["problems"] and stats["host_reads"] == 0
    return stats


@pytest.mark.parametrize("model,probability", [("SVC", False), ("SVC", True), ("SVR", False)])
def test_family_batched_path_equals_loop_on_cpu(model, probability, monkeypatch):
    stats = check_family(family_runs("cpu", model, 240, 2, monkeypatch, probability))
    assert stats["launches"] == check_family(family_runs("cpu", model, 240, 4, monkeypatch, probability))["launches"]


def test_log_loss_scores_agree_on_cpu(monkeypatch):
    assert log_loss_scores("cpu", 240, monkeypatch) <= 1e-9


def test_kept_models_come_back_in_one_batch(monkeypatch):
    rng = np.random.RandomState(3)
    X = rng.randn(150, 4).astype(np.float32)
    y = (X[:, 0] + 0.3 * rng.randn(150) > 0).astype(np.int64)
    models, reads = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DML_SVM_DECISION", mode)
        spec = JobSpec("SVC", [{"C": 1.0}], cv=2, holdout=True, keep_models="all")
        res = run_candidates(DeviceData(X, y, True, "cpu"), spec, [0])
        models[mode] = [m for r in res for m in (r.model or {}).get("machines", [])]
        reads[mode] = family_of("SVC").last_decision_stats["host_reads"]
    assert models["1"] and len(models["1"]) == len(models["0"]) and reads == {"1": 5, "0": None}
    for a, b in zip(models["1"], models["0"]):
        assert np.array_equal(a["sv"], b["sv"]) and np.array_equal(a["coef"], b["coef"]) and a["pair"] == b["pair"]
        assert abs(a["rho"] - b["rho"]) <= 1e-14 * abs(b["rho"])

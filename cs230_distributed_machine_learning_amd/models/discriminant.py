"""QuadraticDiscriminantAnalysis: every (candidate, split) of a job from one pass over the table
(docs/QDA.md).

Every row belongs to one (fold bucket, class) cell, a bucket being the rows with the same role
in every split; ``dml_qda_class_moments`` gives every cell's count, column sums and X^T X in one
launch, and a split's training moments of a class are the sum of the cells its role vector marks
as training rows.  One batched ``eigh`` over all (split, class) covariances gives sklearn's
``scalings_`` (before regularisation) and ``rotations_``; a candidate's ``reg_param`` only changes
the per-component variances, so every candidate of a split shares the projection and
``dml_qda_score`` scores all of them in one pass over the held-out rows.

The CPU data path, a ``d`` above the kernel's limit and a split layout with more than
``MAX_BUCKETS`` buckets run the same formulas in plain float64 torch (``DML_QDA_KERNEL=0`` forces
that path on a GPU: the baseline of scripts/bench_qda.py).

LinearDiscriminantAnalysis (docs/LDA.md) starts from the same cell moments: a split's pooled
within-class covariance is a prior-weighted sum of class covariances, one batched ``eigh`` per
split serves every float ``shrinkage``, ``shrinkage="auto"`` adds the Ledoit-Wolf row statistic
(``dml_lda_lw_stat``), the ``svd`` solver is rebuilt from the moments, and every candidate of every
split is one column of the fused linear scorer ``dml_lda_score`` (``DML_LDA_KERNEL=0``: float64
torch, the baseline of scripts/bench_lda.py).
"""
from __future__ import annotations

import math
import os
import time
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from ..search.cv import ROLE_TRAIN
from ..utils import trace
from .base import Family, FitOutput, FitTask, ParamError, as_bool, as_float, as_int, register

_DEFAULTS = {"priors": None, "reg_param": 0.0, "store_covariance": False, "tol": 1e-4}
MAX_BUCKETS = 64
ONE_SAMPLE = "y has only 1 sample in class {}, covariance is ill defined."
NOT_FULL_RANK = ("The covariance matrix of class {} is not full rank. Increasing the value of parameter "
                 "`reg_param` might help reducing the collinearity.")


def _moments_torch(data, splits: List[int], shift: torch.Tensor) -> torch.Tensor:
    """[len(splits), C, d + 1, d + 1]: every (split, class)'s training moments of
    z = [x - shift, 1] in plain float64 torch."""
    C, d = data.n_classes, data.d
    out = torch.zeros((len(splits), C, d + 1, d + 1), dtype=torch.float64, device=data.device)
    for i, s in enumerate(splits):
        tr = data.train_rows[s].long()
        yt = data.y_cls[tr]
        for c in range(C):
            Z = data.X[tr[yt == c]].double() - shift
            Z = torch.cat([Z, torch.ones((Z.shape[0], 1), dtype=torch.float64, device=Z.device)], 1)
            out[i, c] = Z.t() @ Z
    return out


def _cells(data, splits: List[int]):
    """The rows grouped by (fold bucket, class) cell: (patterns [B, S], perm int32 [n], off int64
    [B * C + 1]), or None when the splits cut the rows into more than MAX_BUCKETS buckets."""
    dev, C = data.device, data.n_classes
    roles = data.roles[torch.tensor(splits, dtype=torch.long, device=dev)]          # [S, n]
    patterns, bucket = torch.unique(roles.t(), dim=0, return_inverse=True)          # [B, S], [n]
    B = int(patterns.shape[0])
    if B > MAX_BUCKETS:
        return None
    cell = bucket * C + data.y_cls.long()
    perm = torch.sort(cell, stable=True).indices.to(torch.int32)
    off = torch.zeros(B * C + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(torch.bincount(cell, minlength=B * C), 0)
    return patterns, perm, off


def _moments_kernel(data, splits: List[int], shift: torch.Tensor, cells=None) -> Optional[torch.Tensor]:
    """The same moments from ONE launch over the table, or None when the splits cut the rows into
    more than MAX_BUCKETS buckets."""
    from ..ops import qda_ops

    cells = cells or _cells(data, splits)
    if cells is None:
        return None
    patterns, perm, off = cells
    B, C = int(patterns.shape[0]), data.n_classes
    M = qda_ops.class_moments(data.X, shift, perm, off)                             # [B * C, d + 1, d + 1]
    train = (patterns.t() == ROLE_TRAIN).double()                                   # [S, B]
    return torch.einsum("sb,bcij->scij", train, M.view(B, C, *M.shape[1:]))


def _eig(M: torch.Tensor, shift: torch.Tensor):
    """From the moments [S, C, d + 1, d + 1]: counts [S, C], means [S, C, d], the descending
    eigenvalues S2 [S, C, d] of every class covariance (n_c - 1 denominator), its rotations
    V [S, C, d, d] (column j = component j) and keep [S, C, d], 1 for the first min(n_c, d)
    components (the ones sklearn's thin SVD of the centred class rows returns)."""
    d = M.shape[-1] - 1
    cnt = M[..., d, d]
    n1 = cnt.clamp_min(1.0)
    dm = M[..., :d, d] / n1.unsqueeze(-1)
    cov = (M[..., :d, :d] - n1[..., None, None] * dm.unsqueeze(-1) * dm.unsqueeze(-2)) / (cnt - 1.0).clamp_min(1.0)[
        ..., None, None]
    lam, V = torch.linalg.eigh(cov)
    S2 = lam.flip(-1).clamp_min(0.0)
    V = V.flip(-1)
    keep = (torch.arange(d, device=M.device) < cnt.unsqueeze(-1)).double()
    return cnt, dm + shift, S2, V * keep.unsqueeze(-2), keep


def _tables(cnt, S2, keep, regs: List[float], priors: List[Optional[List[float]]]):
    """inv [S, NC, C, d], cst [S, NC, C] and the regularised variances S2r [S, NC, C, d] of every
    candidate (reg_param, priors)."""
    dev = S2.device
    r = torch.tensor(regs, dtype=torch.float64, device=dev).view(1, -1, 1, 1)
    S2r = ((1.0 - r) * S2.unsqueeze(1) + r) * keep.unsqueeze(1)
    inv = torch.where(keep.unsqueeze(1) > 0, 1.0 / S2r, torch.zeros_like(S2r))
    logs = torch.where(keep.unsqueeze(1) > 0, torch.log(S2r), torch.zeros_like(S2r)).sum(-1)
    emp = cnt / cnt.sum(-1, keepdim=True).clamp_min(1.0)                             # [S, C]
    pri = torch.stack([emp if p is None else torch.tensor(p, dtype=torch.float64, device=dev).expand_as(emp)
                       for p in priors], 1)                                          # [S, NC, C]
    return inv, -0.5 * logs + torch.log(pri), S2r


def _score_torch(data, splits, mu, V, inv, cst):
    """(pred [NC, total] int32, dec [NC, total, C]) in float64 torch: per split and class one
    projection of the held-out rows, shared by the candidates."""
    preds, decs = [], []
    for i, s in enumerate(splits):
        Xt = data.X[data.test_rows[s].long()].double()
        cols = []
        for c in range(mu.shape[1]):
            Z = (Xt - mu[i, c]) @ V[i, c]
            cols.append(cst[i, :, c].unsqueeze(1) - 0.5 * ((Z * Z) @ inv[i, :, c].t()).t())   # [NC, m]
        dec = torch.stack(cols, -1)
        decs.append(dec)
        preds.append(dec.argmax(-1).to(torch.int32))
    return torch.cat(preds, 1), torch.cat(decs, 1)


class DiscriminantFamily(Family):
    model_types = ("QuadraticDiscriminantAnalysis",)
    classifiers = ("QuadraticDiscriminantAnalysis",)
    data_parallel = False   # no row-sharded moments: such a job runs task-parallel
    streams_rows = False

    def resolve(self, model_type, params, n_train, n_features, n_classes):
        p = dict(_DEFAULTS)
        p.update({k: v for k, v in params.items() if k in _DEFAULTS})
        warn = []
        unknown = sorted(k for k in params if k not in _DEFAULTS)
        if unknown:
            warn.append(f"ignored unknown parameters {unknown}")
        try:
            reg = as_float(p["reg_param"], "reg_param", lo=0.0, hi=1.0)
        except ParamError:
            raise ParamError(f"The 'reg_param' parameter of {model_type} must be a float in the range [0.0, 1.0]. "
                             f"Got {p['reg_param']!r} instead.") from None
        tol = as_float(p["tol"], "tol", lo=0.0)
        as_bool(p["store_covariance"], "store_covariance")   # accepted; a CV fit stores no covariance
        priors = p["priors"]
        if priors is not None:
            try:
                priors = [float(v) for v in priors]
            except (TypeError, ValueError):
                raise ParamError(f"priors must be None or a sequence of {n_classes} floats, got {p['priors']!r}") from None
            if len(priors) != n_classes or any(math.isnan(v) or v < 0 for v in priors):
                raise ParamError(f"priors must be None or a sequence of {n_classes} non-negative floats, "
                                 f"got {p['priors']!r}")
        return {"reg_param": reg, "tol": tol, "priors": priors, "warnings": warn}

    def cost(self, model_type, rp, n_train, n_features, n_classes) -> float:
        d2 = n_features * n_features
        return (n_train * d2 + (n_train / 4.0) * max(1, n_classes) * d2) * 2e-12 + 1e-3

    @staticmethod
    def use_kernel(data) -> bool:
        if not data.is_gpu or os.environ.get("DML_QDA_KERNEL", "1") == "0":
            return False
        from ..ops import qda_ops

        return data.d <= qda_ops.max_d()

    def run(self, data, tasks: List[FitTask], keep_models: bool = False) -> List[FitOutput]:
        if not tasks:
            return []
        if not data.classification:
            raise ParamError(f"{tasks[0].model_type} needs a classification target")
        if data.X is None:
            raise ParamError("QuadraticDiscriminantAnalysis needs the float32 rows (this table arrived as bins only)")
        t0 = time.perf_counter()
        dev, C, d = data.device, data.n_classes, data.d
        splits = sorted({t.split for t in tasks})
        kernel = self.use_kernel(data)
        shift = torch.mean(data.X, 0, dtype=torch.float64)
        with trace.range("qda_moments"):
            M = _moments_kernel(data, splits, shift) if kernel else None
            if M is None:
                M = _moments_torch(data, splits, shift)
        with trace.range("qda_eigh"):
            cnt, mu, S2, V, keep = _eig(M, shift)
        cands: Dict[Any, int] = {}
        cand_of = []
        for t in tasks:
            key = (t.params["reg_param"], None if t.params["priors"] is None else tuple(t.params["priors"]))
            cand_of.append(cands.setdefault(key, len(cands)))
        keys = list(cands)
        inv, cst, S2r = _tables(cnt, S2, keep, [k[0] for k in keys], [None if k[1] is None else list(k[1]) for k in keys])
        want_dec = any(t.need_proba or (keep_models and t.keep) for t in tasks)
        off = np.concatenate([[0], np.cumsum([int(data.test_rows[s].numel()) for s in splits])]).astype(np.int64)
        with trace.range("qda_score"):
            if off[-1] == 0:
                pred = torch.zeros((len(keys), 0), dtype=torch.int32, device=dev)
                dec = torch.zeros((len(keys), 0, C), dtype=torch.float64, device=dev)
            elif kernel:
                from ..ops import qda_ops

                rows = torch.cat([data.test_rows[s] for s in splits])
                step = qda_ops.max_candidates()
                parts = [qda_ops.score(data.X, rows, off, mu, V, inv[:, k:k + step], cst[:, k:k + step], want_dec)
                         for k in range(0, len(keys), step)]
                pred = torch.cat([p for p, _d in parts])
                dec = torch.cat([dd for _p, dd in parts]) if want_dec else None
            else:
                pred, dec = _score_torch(data, splits, mu, V, inv, cst)
        # what the host needs: the class counts, and every candidate's rank per (split, class)
        tols = torch.tensor([t.params["tol"] for t in tasks], dtype=torch.float64, device=dev)
        sp_of = torch.tensor([splits.index(t.split) for t in tasks], device=dev)
        cd_of = torch.tensor(cand_of, device=dev)
        rank = ((S2r[sp_of, cd_of] > tols.view(-1, 1, 1)) & (keep[sp_of] > 0)).sum(-1)      # [tasks, C]
        cnt_h, rank_h = cnt.cpu().numpy(), rank.cpu().numpy()
        outs = []
        for i, t in enumerate(tasks):
            si, k = splits.index(t.split), cand_of[i]
            warn = list(t.params.get("warnings", []))
            o = FitOutput(task_id=t.task_id, info={"warnings": warn})
            outs.append(o)
            one = [c for c in range(C) if cnt_h[si, c] == 1]
            if one:
                o.error = ONE_SAMPLE.format(data.classes[one[0]])
                continue
            warn.extend(NOT_FULL_RANK.format(c) for c in range(C) if cnt_h[si, c] > 1 and rank_h[i, c] < d)
            a, b = int(off[si]), int(off[si + 1])
            o.pred = pred[k, a:b]
            if dec is not None and t.need_proba:
                o.proba = torch.softmax(dec[k, a:b], -1).float()
            if keep_models and t.keep:
                pri = (cnt[si] / cnt[si].sum()) if t.params["priors"] is None else torch.tensor(t.params["priors"])
                o.model = {"kind": "qda", "model_type": t.model_type, "classes": np.asarray(data.classes),
                           "priors": pri.double().cpu().numpy(), "means": mu[si].cpu().numpy(),
                           "rotations": V[si].cpu().numpy(), "scalings": S2r[si, k].cpu().numpy(),
                           "n_kept": np.minimum(cnt_h[si], d).astype(np.int64),
                           "reg_param": float(t.params["reg_param"]), "tol": float(t.params["tol"])}
        if data.is_gpu:
            torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        for o in outs:
            o.fit_seconds = dt / len(outs)
        return outs


def qda_decision_numpy(model: Dict[str, Any], X: np.ndarray) -> np.ndarray:
    """sklearn's ``_decision_function`` [n, C] of a kept model, numpy float64."""
    X = np.asarray(X, dtype=np.float64)
    cols = []
    for c in range(len(model["priors"])):
        k = int(model["n_kept"][c])
        S = np.asarray(model["scalings"], dtype=np.float64)[c, :k]
        R = np.asarray(model["rotations"], dtype=np.float64)[c][:, :k]
        X2 = (X - np.asarray(model["means"], dtype=np.float64)[c]) @ (R * S ** -0.5)
        cols.append(-0.5 * ((X2 ** 2).sum(1) + np.log(S).sum()))
    with np.errstate(divide="ignore"):
        return np.stack(cols, 1) + np.log(np.asarray(model["priors"], dtype=np.float64))


register(DiscriminantFamily())


# ---- LinearDiscriminantAnalysis (docs/LDA.md) --------------------------------------------------
_LDA_DEFAULTS = {"solver": "svd", "shrinkage": None, "priors": None, "n_components": None,
                 "store_covariance": False, "tol": 1e-4, "covariance_estimator": None}
SVD_SHRINKAGE = "shrinkage not supported with 'svd' solver."
BAD_COMPONENTS = "n_components cannot be larger than min(n_features, n_classes - 1)."
PRIORS_RENORM = "The priors do not sum to 1. Renormalizing"
NOT_POSITIVE_DEFINITE = ("The leading minor of order {} of B is not positive definite. The factorization of B could "
                         "not be completed and no eigenvalues or eigenvectors were computed.")
_EPS = float(np.finfo(np.float64).eps)


def _class_stats(M: torch.Tensor, shift: torch.Tensor):
    """From the moments [S, C, d + 1, d + 1]: counts [S, C], class means [S, C, d] and the biased
    class covariances emp [S, C, d, d] (divided by n_c)."""
    d = M.shape[-1] - 1
    cnt = M[..., d, d]
    n1 = cnt.clamp_min(1.0)
    dm = M[..., :d, d] / n1.unsqueeze(-1)
    emp = M[..., :d, :d] / n1[..., None, None] - dm.unsqueeze(-1) * dm.unsqueeze(-2)
    return cnt, dm + shift, emp


def _lw_stat_torch(data, splits, mu, w) -> torch.Tensor:
    """beta_ [S, C] of Ledoit-Wolf in float64 torch: per (split, class) the sum over the class's
    training rows of (sum_j w_j (x_j - m_j)^2)^2."""
    out = torch.zeros(mu.shape[:2], dtype=torch.float64, device=mu.device)
    for i, s in enumerate(splits):
        tr = data.train_rows[s].long()
        yt = data.y_cls[tr]
        for c in range(mu.shape[1]):
            Z = data.X[tr[yt == c]].double() - mu[i, c]
            q = (Z * Z) @ w[i, c]
            out[i, c] = (q * q).sum()
    return out


def _ledoit_wolf(cnt, emp, beta_):
    """sklearn's ``_cov(X, "auto")`` of every (split, class) from its moments and beta_: the
    Ledoit-Wolf covariance of the standardised rows, scaled back.  Returns [S, C, d, d]."""
    d = emp.shape[-1]
    var = torch.diagonal(emp, dim1=-2, dim2=-1).clamp_min(0.0)
    var = torch.where(var > 0, var, torch.ones_like(var))          # a zero standard deviation is replaced by 1
    sd = var.sqrt()
    R = emp / (sd.unsqueeze(-1) * sd.unsqueeze(-2))
    n = cnt.clamp_min(1.0)
    delta_ = (R * R).sum((-2, -1))
    tr = torch.diagonal(R, dim1=-2, dim2=-1).sum(-1)
    m = tr / d
    beta = (beta_ / n - delta_) / (d * n)
    delta = (delta_ - 2.0 * m * tr + d * m * m) / d
    beta = torch.minimum(beta, delta)
    sh = torch.where((beta == 0) | (delta <= 0), torch.zeros_like(beta), beta / delta)
    if d == 1:
        sh = torch.zeros_like(sh)
    eye = torch.eye(d, dtype=torch.float64, device=emp.device)
    return (1.0 - sh)[..., None, None] * emp + (sh * m)[..., None, None] * (var.unsqueeze(-1) * eye)


def _solve(lam, U, mu, logp):
    """coef [S, C, d] = mu Sigma^+ and intercept [S, C] from Sigma's eigenvalues lam [S, d] and
    eigenvectors U: eigenvalues below eps x the largest are dropped (the minimum-norm solution)."""
    top = lam.max(-1, keepdim=True).values
    keep = lam > _EPS * top
    inv = torch.where(keep, 1.0 / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
    W = ((mu @ U) * inv.unsqueeze(-2)) @ U.transpose(-1, -2)
    return W, -0.5 * (mu * W).sum(-1) + logp


def _svd_solver(cnt, mu, emp, pri, tol: float):
    """sklearn's ``_solve_svd`` from the moments: (coef [S, C, d], intercept [S, C])."""
    C = mu.shape[1]
    N = cnt.sum(-1)
    scatter = (cnt[..., None, None] * emp).sum(1)
    std = (torch.diagonal(scatter, dim1=-2, dim2=-1).clamp_min(0.0) / N.unsqueeze(-1)).sqrt()
    std = torch.where(std == 0, torch.ones_like(std), std)
    G = scatter / (std.unsqueeze(-1) * std.unsqueeze(-2)) / (N - C).clamp_min(1.0)[:, None, None]
    lam, V = torch.linalg.eigh(G)
    sv = lam.flip(-1).clamp_min(0.0).sqrt()                          # sklearn's singular values, descending
    keep = sv > tol
    scal = V.flip(-1) / std.unsqueeze(-1) * torch.where(keep, 1.0 / sv.clamp_min(1e-300), torch.zeros_like(sv)).unsqueeze(-2)
    xbar = (pri.unsqueeze(-1) * mu).sum(1)
    fac = 1.0 if C == 1 else 1.0 / (C - 1)
    dm = mu - xbar.unsqueeze(1)
    _, s2, Vt = torch.linalg.svd(((N.unsqueeze(-1) * pri * fac).sqrt().unsqueeze(-1) * dm) @ scal, full_matrices=False)
    sc = scal @ (Vt.transpose(-1, -2) * (s2 > tol * s2[:, :1]).double().unsqueeze(-2))
    proj = dm @ sc
    W = proj @ sc.transpose(-1, -2)
    return W, -0.5 * (proj * proj).sum(-1) + torch.log(pri) - (xbar.unsqueeze(1) * W).sum(-1)


class LinearDiscriminantFamily(Family):
    model_types = ("LinearDiscriminantAnalysis",)
    classifiers = ("LinearDiscriminantAnalysis",)
    data_parallel = False   # no row-sharded moments: such a job runs task-parallel
    streams_rows = False

    def resolve(self, model_type, params, n_train, n_features, n_classes):
        p = dict(_LDA_DEFAULTS)
        p.update({k: v for k, v in params.items() if k in _LDA_DEFAULTS})
        warn = []
        unknown = sorted(k for k in params if k not in _LDA_DEFAULTS)
        if unknown:
            warn.append(f"ignored unknown parameters {unknown}")
        solver = p["solver"]
        if solver not in ("svd", "lsqr", "eigen"):
            raise ParamError(f"The 'solver' parameter of {model_type} must be a str among {{'svd', 'lsqr', 'eigen'}}. "
                             f"Got {solver!r} instead.")
        shrinkage = p["shrinkage"]
        if shrinkage is not None and shrinkage != "auto":
            try:
                if isinstance(shrinkage, str):
                    raise ParamError("str")
                shrinkage = as_float(shrinkage, "shrinkage", lo=0.0, hi=1.0)
            except ParamError:
                raise ParamError(f"The 'shrinkage' parameter of {model_type} must be a str among {{'auto'}}, a float in "
                                 f"the range [0.0, 1.0] or None. Got {p['shrinkage']!r} instead.") from None
        if p["covariance_estimator"] is not None:
            raise ParamError("covariance_estimator is not supported: it must be None")
        tol = as_float(p["tol"], "tol", lo=0.0)
        store = as_bool(p["store_covariance"], "store_covariance")
        priors = p["priors"]
        if priors is not None:
            try:
                priors = [float(v) for v in priors]
            except (TypeError, ValueError):
                raise ParamError(f"priors must be None or a sequence of {n_classes} floats, got {p['priors']!r}") from None
            if len(priors) != n_classes or any(math.isnan(v) for v in priors):
                raise ParamError(f"priors must be None or a sequence of {n_classes} floats, got {p['priors']!r}")
            if any(v < 0 for v in priors):
                raise ParamError("priors must be non-negative")
            if abs(sum(priors) - 1.0) > 1e-5:
                warn.append(PRIORS_RENORM)
                total = float(np.sum(priors))
                priors = [v / total for v in priors]
        nc = as_int(p["n_components"], "n_components", lo=1, allow_none=True)
        if nc is not None and nc > min(n_classes - 1, n_features):
            raise ParamError(BAD_COMPONENTS)
        return {"solver": solver, "shrinkage": shrinkage, "tol": tol, "priors": priors, "store_covariance": store,
                "warnings": warn}

    def cost(self, model_type, rp, n_train, n_features, n_classes) -> float:
        # the moments pass and the d^3 solve are shared by a split's candidates; a fit's own share is
        # its linear scores over the held-out rows (and, for "auto", one more pass over the rows)
        d2 = n_features * n_features
        rows = n_train * n_features * (2.0 if rp.get("shrinkage") == "auto" else 1.0)
        return (n_train * d2 + rows + (n_train / 4.0) * max(1, n_classes) * n_features) * 2e-12 + 1e-3

    @staticmethod
    def use_kernel(data) -> bool:
        if not data.is_gpu or os.environ.get("DML_LDA_KERNEL", "1") == "0":
            return False
        from ..ops import lda_ops

        return data.d <= lda_ops.max_d()

    def run(self, data, tasks: List[FitTask], keep_models: bool = False) -> List[FitOutput]:
        if not tasks:
            return []
        if not data.classification:
            raise ParamError(f"{tasks[0].model_type} needs a classification target")
        if data.X is None:
            raise ParamError("LinearDiscriminantAnalysis needs the float32 rows (this table arrived as bins only)")
        from ..ops import lda_ops

        t0 = time.perf_counter()
        dev, C, d = data.device, data.n_classes, data.d
        splits = sorted({t.split for t in tasks})
        S = len(splits)
        cells = _cells(data, splits) if self.use_kernel(data) else None
        kernel = cells is not None
        shift = torch.mean(data.X, 0, dtype=torch.float64)
        with trace.range("lda_moments"):
            M = _moments_kernel(data, splits, shift, cells) if kernel else _moments_torch(data, splits, shift)
        cnt, mu, emp = _class_stats(M, shift)
        freq = cnt / cnt.sum(-1, keepdim=True).clamp_min(1.0)
        pri_of = lambda pk: freq if pk is None else torch.tensor(pk, dtype=torch.float64, device=dev).expand(S, C)
        live = [t for t in tasks if not (t.params["solver"] == "svd" and t.params["shrinkage"] is not None)]
        pkey = lambda t: None if t.params["priors"] is None else tuple(t.params["priors"])
        cov_auto = None
        if any(t.params["shrinkage"] == "auto" for t in live):
            with trace.range("lda_lw_stat"):
                var = torch.diagonal(emp, dim1=-2, dim2=-1).clamp_min(0.0)
                w = 1.0 / torch.where(var > 0, var, torch.ones_like(var))
                if kernel:
                    patterns, perm, off = cells
                    train = patterns == ROLE_TRAIN                                               # [B, S]
                    stat = lda_ops.lw_stat(data.X, perm, off, train, mu, w)                      # [B * C, S]
                    beta_ = torch.einsum("bs,bcs->sc", train.double(), stat.view(-1, C, S))
                else:
                    beta_ = _lw_stat_torch(data, splits, mu, w)
                cov_auto = _ledoit_wolf(cnt, emp, beta_)
        # one scoring column per distinct (shrinkage, priors) of lsqr / eigen and (tol, priors) of svd
        cols: Dict[Any, int] = {}
        col_of = {}
        for t in live:
            key = (("svd", t.params["tol"]) if t.params["solver"] == "svd" else ("sh", t.params["shrinkage"])) + (pkey(t),)
            col_of[t.task_id] = cols.setdefault(key, len(cols))
        eig: Dict[Any, Any] = {}      # priors key (and "auto") -> eigh of the pooled covariance

        def pooled(pk, auto):
            k = (pk, auto)
            if k not in eig:
                Sw = (pri_of(pk)[..., None, None] * (cov_auto if auto else emp)).sum(1)
                eig[k] = (Sw,) + tuple(torch.linalg.eigh(Sw))
            return eig[k]

        def sigma(key):
            kind, a, pk = key
            if kind == "svd" or a is None or a == "auto":
                return pooled(pk, a == "auto" and kind != "svd")[0]
            Sw = pooled(pk, False)[0]
            m = torch.diagonal(Sw, dim1=-2, dim2=-1).sum(-1) / d
            return (1.0 - a) * Sw + (a * m)[:, None, None] * torch.eye(d, dtype=torch.float64, device=dev)

        Ws, bs = [], []
        with trace.range("lda_solve"):
            for kind, a, pk in cols:
                pri = pri_of(pk)
                if kind == "svd":
                    W, b = _svd_solver(cnt, mu, emp, pri, a)
                else:
                    _Sw, lam, U = pooled(pk, a == "auto")
                    if a is not None and a != "auto":
                        lam = (1.0 - a) * lam + a * lam.sum(-1, keepdim=True) / d
                    W, b = _solve(lam, U, mu, torch.log(pri))
                Ws.append(W)
                bs.append(b)
        keys = list(cols)
        want_dec = any(t.need_proba for t in live)
        off = np.concatenate([[0], np.cumsum([int(data.test_rows[s].numel()) for s in splits])]).astype(np.int64)
        pred = dec = None
        if keys and off[-1] > 0:
            with trace.range("lda_score"):
                W_all, b_all = torch.stack(Ws, 2), torch.stack(bs, 2)               # [S, C, NC, d], [S, C, NC]
                rows = torch.cat([data.test_rows[s] for s in splits])
                if kernel:
                    pred, dec = lda_ops.score(data.X, rows, off, W_all, b_all, want_dec)
                else:
                    pred, dec = lda_ops.score_torch(data.X, rows, [int(v) for v in off], W_all, b_all)
        # eigen fits fail, as scipy's eigh(Sb, Sw) does, where the covariance has no Cholesky factor
        bad = {}
        for key in {keys[col_of[t.task_id]] for t in live if t.params["solver"] == "eigen"}:
            bad[key] = torch.linalg.cholesky_ex(sigma(key)).info.cpu().numpy()
        outs = []
        for t in tasks:
            o = FitOutput(task_id=t.task_id, info={"warnings": list(t.params.get("warnings", []))})
            outs.append(o)
            if t.task_id not in col_of:
                o.error = SVD_SHRINKAGE
                continue
            si, k = splits.index(t.split), col_of[t.task_id]
            if t.params["solver"] == "eigen" and bad[keys[k]][si] > 0:
                o.error = NOT_POSITIVE_DEFINITE.format(int(bad[keys[k]][si]))
                continue
            lo, hi = int(off[si]), int(off[si + 1])
            o.pred = pred[k, lo:hi] if pred is not None else torch.zeros(0, dtype=torch.int32, device=dev)
            if t.need_proba:
                o.proba = (torch.softmax(dec[k, lo:hi], -1).float() if dec is not None
                           else torch.zeros((0, C), dtype=torch.float32, device=dev))
            if keep_models and t.keep:
                o.model = {"kind": "lda", "model_type": t.model_type, "classes": np.asarray(data.classes),
                           "solver": t.params["solver"], "priors": pri_of(keys[k][2])[si].cpu().numpy(),
                           "means": mu[si].cpu().numpy(), "coef": Ws[k][si].cpu().numpy(),
                           "intercept": bs[k][si].cpu().numpy()}
                if t.params["solver"] != "svd" or t.params["store_covariance"]:
                    o.model["covariance"] = sigma(keys[k])[si].cpu().numpy()
        if data.is_gpu:
            torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        for o in outs:
            o.fit_seconds = dt / len(outs)
        return outs


def lda_decision_numpy(model: Dict[str, Any], X: np.ndarray) -> np.ndarray:
    """The class scores [n, C] of a kept model, numpy float64 (for two classes sklearn's
    ``decision_function`` is column 1 minus column 0)."""
    return np.asarray(X, dtype=np.float64) @ np.asarray(model["coef"], dtype=np.float64).T + np.asarray(
        model["intercept"], dtype=np.float64)


register(LinearDiscriminantFamily())

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
from .base import Family, FitOutput, FitTask, ParamError, as_bool, as_float, register

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


def _moments_kernel(data, splits: List[int], shift: torch.Tensor) -> Optional[torch.Tensor]:
    """The same moments from ONE launch over the table, or None when the splits cut the rows into
    more than MAX_BUCKETS buckets."""
    from ..ops import qda_ops

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

"""Per-stage statistics of gradient-boosting fits (docs/GBRT_STAGED.md).

``stage_stats`` reduces, for every recorded fit of a batch and in one launch, the loss sum and
the score statistic of the fit's in-bag, out-of-bag and held-out rows from the raw scores a stage
has just written: csrc/kernels/gbrt.hip ``k_gb_stage_stats`` / ``k_gb_stage_stats_reduce`` on the
GPU, csrc/runtime/gbrt_stats_cpu.cpp on the host (same definition, same summation order).
Nothing is read back: the statistics of every stage land in one ``stats`` tensor that
``stage_curves`` turns into sklearn's numbers (``train_score_``, ``oob_scores_``, the staged CV
score) after the stage loop.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Optional

import numpy as np
import torch

from ..utils import native
from .forest_ops import PERM_SCORERS

# csrc/kernels/gbrt.hip GbLoss == models/boosting.py LOSS_*
LOSS_SQ, LOSS_ABS, LOSS_HUBER, LOSS_QUANT, LOSS_LOG, LOSS_EXP = range(6)
CAT_INBAG, CAT_OOB, CAT_TEST = 0, 1, 2
MAX_FITS = 65535   # grid.y of one launch


def new_stats(n_fits: int, n_stages: int, device) -> torch.Tensor:
    """``stats`` [n_fits][n_stages][3 categories][3]: {n int64, match count int64 (classification)
    or SSE double bits (regression), loss sum double bits}, zeroed."""
    return torch.zeros((n_fits, n_stages, 3, 3), dtype=torch.int64, device=device)


def stats_plan(fit_raw, fit_loss, fit_role, fit_inbag, fit_val, fit_out, fit_dpos, alpha, *, K: int, raw_rows: int,
               role_rows: int, inbag_rows: int, val_rows: int, stat_fits: int, delta_len: int, device) -> Dict[str, Any]:
    """The per-fit index arrays of a launch, checked on the host against the shapes they index
    (the kernel trusts them) and uploaded once; a launch plan lives as long as its active set."""
    cols = [np.asarray(c, dtype=np.int64).reshape(-1) for c in (fit_raw, fit_loss, fit_role, fit_inbag, fit_val,
                                                                 fit_out, fit_dpos)]
    A = len(cols[0])
    if any(len(c) != A for c in cols) or len(np.asarray(alpha).reshape(-1)) != A:
        raise ValueError("stage statistics: the per-fit arrays must have one entry per fit")
    lim = [(0, raw_rows - K), (0, 5), (0, role_rows - 1), (0, inbag_rows - 1), (-1, val_rows - 1), (0, stat_fits - 1),
           (0, max(delta_len - 1, 0))]
    names = ("fit_raw", "fit_loss", "fit_role", "fit_inbag", "fit_val", "fit_out", "fit_dpos")
    for name, c, (lo, hi) in zip(names, cols, lim):
        if A and (c.min() < lo or c.max() > hi):
            raise ValueError(f"stage statistics: {name} out of range [{lo}, {hi}]")
    if A and K > 1 and not np.isin(cols[1], (LOSS_LOG,)).all():
        raise ValueError("stage statistics: K > 1 is the multinomial log-loss")
    tab = torch.from_numpy(np.stack(cols).astype(np.int32)).to(device)   # [7][A]
    al = torch.from_numpy(np.asarray(alpha, dtype=np.float64).reshape(-1).copy()).to(device)
    return {"A": A, "tab": tab, "alpha": al, "K": int(K), "stat_fits": stat_fits, "has_val": bool(val_rows > 0)}


def part_words(n: int, A: int) -> int:
    """Words of the ``part`` scratch: 9 per fit for every 256-row block, then for every group of
    each level of the 16-to-1 reduction but the last."""
    E, units = min(A, MAX_FITS) * 9, (n + 255) // 256
    total = units
    while units > 16:
        units = (units + 15) // 16
        total += units
    return total * E


def stage_stats(raw: torch.Tensor, y: torch.Tensor, roles: torch.Tensor, inbag: torch.Tensor,
                val_mask: Optional[torch.Tensor], plan: Dict[str, Any], delta: Optional[torch.Tensor],
                stats: torch.Tensor, stage: int, part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One stage's statistics of the plan's fits into ``stats[:, stage]``.

    raw float64 [F * K][n] (or [F][K][n]); y int32 [n] class ids for log_loss / exponential fits,
    float64 [n] targets for the regression losses; roles uint8 [n_splits][n] (search/cv.py
    ROLE_*); inbag uint8 [rows][n]; val_mask uint8 [rows][n] or None; delta float64 huber deltas
    or None.  Dispatches by device: the HIP kernels on the GPU (the current stream), the host twin
    on the CPU.  Returns ``part``, the block partials [blocks][A][3][3] of the last launch."""
    n = int(raw.shape[-1])
    A, K, tab = plan["A"], plan["K"], plan["tab"]
    dev = raw.device
    for name, t, dt in (("raw", raw, torch.float64), ("roles", roles, torch.uint8), ("inbag", inbag, torch.uint8),
                        ("stats", stats, torch.int64)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"stage statistics: {name} must be a contiguous {dt} tensor on {dev}")
    if roles.shape[-1] != n or inbag.shape[-1] != n or (val_mask is not None and val_mask.shape[-1] != n) \
            or y.shape[-1] != n:
        raise ValueError("stage statistics: every row array must have n columns")
    if val_mask is not None and (val_mask.dtype != torch.uint8 or not val_mask.is_contiguous()):
        raise ValueError("stage statistics: val_mask must be a contiguous uint8 tensor")
    if plan["has_val"] != (val_mask is not None):
        raise ValueError("stage statistics: the plan and the call disagree on the validation masks")
    is_cls = y.dtype == torch.int32
    if not is_cls and y.dtype != torch.float64:
        raise ValueError("stage statistics: y is int32 class ids or float64 targets")
    n_stages = int(stats.shape[1])
    if stats.shape[0] != plan["stat_fits"] or tuple(stats.shape[2:]) != (3, 3) or not 0 <= stage < n_stages:
        raise ValueError("stage statistics: stats is [fits][stages][3][3] and stage one of its stages")
    need = part_words(n, A)
    if part is None or part.numel() < need:
        part = torch.empty(max(need, 1), dtype=torch.int64, device=dev)
    if A == 0 or n == 0:
        return part
    gpu = dev.type == "cuda"
    lib = native.hip_lib() if gpu else native.cpu_lib()
    if gpu and getattr(lib, "dml_gb_stage_stats", None) is None:
        raise RuntimeError("the HIP library has no dml_gb_stage_stats: rebuild it")
    for a0 in range(0, A, MAX_FITS):   # grid.y limit
        a1 = min(A, a0 + MAX_FITS)
        col = [native.ptr(tab[i]) + 4 * a0 for i in range(7)]
        common = dict(n=n, K=K, A=a1 - a0, raw=native.ptr(raw), ycls=native.ptr(y) if is_cls else 0,
                      yreg=0 if is_cls else native.ptr(y), roles=native.ptr(roles), inbag=native.ptr(inbag),
                      val=native.ptr(val_mask), fit_raw=col[0], fit_loss=col[1], fit_role=col[2], fit_inbag=col[3],
                      fit_val=col[4], fit_out=col[5], fit_dpos=col[6], fit_alpha=native.ptr(plan["alpha"]) + 8 * a0,
                      delta=native.ptr(delta), part=native.ptr(part), stats=native.ptr(stats), stage=stage,
                      n_stages=n_stages)
        if gpu:
            args = native.GbStatsArgs(**common)
            rc = lib.dml_gb_stage_stats(ctypes.byref(args), native.stream_handle(dev))
            if rc:
                raise RuntimeError(f"dml_gb_stage_stats failed ({rc})")
        else:
            lib.dml_cpu_gbrt_stage_stats(*[common[k] for k in (
                "n", "K", "A", "raw", "ycls", "yreg", "roles", "inbag", "val", "fit_raw", "fit_loss", "fit_role",
                "fit_inbag", "fit_val", "fit_out", "fit_dpos", "fit_alpha", "delta", "part", "stats", "stage",
                "n_stages")])
    return part


def stats_arrays(stats, is_cls: bool):
    """(n int64, score statistic, loss sum float64) of a host copy of ``stats`` [..., 3, 3]: the
    statistic is the match count (int64) for classifiers, the squared-error sum for regressors."""
    st = np.ascontiguousarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    cnt = st[..., 0]
    stat = st[..., 1] if is_cls else np.ascontiguousarray(st[..., 1]).view(np.float64)
    return cnt, stat, np.ascontiguousarray(st[..., 2]).view(np.float64)


def loss_factor(loss: int, K: int) -> float:
    """sklearn ``_gb.py`` ``_fit_stages``: the half losses of squared_error and binary log_loss
    are doubled in ``train_score_`` / ``oob_scores_`` (backward compatibility)."""
    return 2.0 if loss == LOSS_SQ or (loss == LOSS_LOG and K == 1) else 1.0


def stage_curves(stats, loss: int, K: int, scoring: Optional[str] = None,
                 ss_tot: Optional[float] = None) -> Dict[str, Any]:
    """One fit's ``stats`` [S][3][3] (host or device) as sklearn's per-stage numbers, float64 [S]
    each: ``train_loss`` / ``oob_loss`` / ``test_loss`` = factor * loss sum / n of the category
    (NaN for an empty one) and ``test_score`` under ``scoring`` (``PERM_SCORERS``; None: accuracy
    / r2), with the formulas of ``forest_ops.permutation_importance`` (r2 against ``ss_tot`` =
    the held-out rows' sum (y - mean y)^2; a constant target scores 1 or 0)."""
    is_cls = loss in (LOSS_LOG, LOSS_EXP)
    is_reg = not is_cls
    name = scoring if scoring not in (None, "None", "") else PERM_SCORERS[is_reg][0]
    if name not in PERM_SCORERS[is_reg]:
        raise ValueError(f"staged scoring must be one of {list(PERM_SCORERS[is_reg])}, got {name!r}")
    cnt, stat, lsum = stats_arrays(stats, is_cls)
    nf = cnt.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_loss = np.where(cnt > 0, loss_factor(loss, K) * lsum / nf, np.nan)
        s, m = stat[:, CAT_TEST].astype(np.float64), nf[:, CAT_TEST]
        if name == "accuracy":
            sc = s / m
        elif name == "r2":
            if ss_tot is None:
                raise ValueError("r2 needs ss_tot")
            sc = np.where(s == 0.0, 1.0, 0.0) if ss_tot == 0.0 else 1.0 - s / ss_tot
        elif name == "neg_mean_squared_error":
            sc = -(s / m)
        else:
            sc = -np.sqrt(s / m)
        sc = np.where(m > 0, sc, np.nan)
    return {"train_loss": mean_loss[:, CAT_INBAG], "oob_loss": mean_loss[:, CAT_OOB],
            "test_loss": mean_loss[:, CAT_TEST], "test_score": sc, "scoring": name,
            "n": cnt.copy()}

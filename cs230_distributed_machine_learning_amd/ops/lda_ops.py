"""LinearDiscriminantAnalysis kernels over torch tensors on either device (docs/LDA.md).

``lw_stat`` and ``score`` run csrc/kernels/lda.hip (``dml_lda_lw_stat``, ``dml_lda_score``) on GPU
tensors and a plain float64 torch implementation of the same formulas on CPU tensors.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from ..utils import native
from .qda_ops import default_parts


class LdaTooLarge(RuntimeError):
    """``d`` is above the kernel's limit; nothing was launched."""


def max_d() -> int:
    return int(native.hip_lib().dml_lda_max_d())


def max_candidates() -> int:
    return int(native.hip_lib().dml_lda_max_candidates())


def max_splits() -> int:
    return int(native.hip_lib().dml_lda_max_splits())


def _check(rc: int, what: str) -> None:
    if rc == native.LDA_TOO_LARGE:
        raise LdaTooLarge(f"{what}: d is above the kernel's limit")
    if rc:
        raise (ValueError if rc == 2 else RuntimeError)(f"{what} failed ({rc})")


def lw_stat(X: torch.Tensor, perm: torch.Tensor, cell_off: torch.Tensor, train: torch.Tensor, mean: torch.Tensor,
            w: torch.Tensor, parts: Optional[int] = None) -> torch.Tensor:
    """[n_cells, S] float64: ``stat[cell, s]`` = sum over rows ``perm[cell_off[cell]:cell_off[cell + 1]]``
    of ``(sum_j w[s, c, j] (x_j - mean[s, c, j])^2)^2`` where ``train[cell // C, s]`` is set, else 0;
    cell = bucket * C + c.  ``X`` float32 [n, d]; ``perm`` int32; ``cell_off`` int64 [n_cells + 1];
    ``train`` [n_cells / C, S]; ``mean`` and ``w`` [S, C, d]."""
    dev = X.device
    n, d = int(X.shape[0]), int(X.shape[1])
    X = X.contiguous()
    if X.dtype != torch.float32:
        raise ValueError("lw_stat: X must be float32")
    S, C = int(mean.shape[0]), int(mean.shape[1])
    perm = perm.to(device=dev, dtype=torch.int32).contiguous()
    cell_off = cell_off.to(device=dev, dtype=torch.int64).contiguous()
    n_cells = int(cell_off.shape[0]) - 1
    train = train.to(device=dev, dtype=torch.int32).contiguous()
    mean = mean.to(device=dev, dtype=torch.float64).contiguous()
    w = w.to(device=dev, dtype=torch.float64).contiguous()
    if (mean.shape != (S, C, d) or w.shape != (S, C, d) or perm.shape != (n,) or C < 1 or n_cells % C
            or train.shape != (n_cells // C, S)):
        raise ValueError("lw_stat: perm [n], cell_off [B C + 1], train [B, S], mean and w [S, C, d] expected")
    out = torch.zeros((n_cells, S), dtype=torch.float64, device=dev)
    if not X.is_cuda:
        cls = torch.arange(n_cells) % C
        off = cell_off.tolist()
        for cell in range(n_cells):
            Z = X[perm[off[cell]:off[cell + 1]].long()].double().unsqueeze(0) - mean[:, cls[cell]].unsqueeze(1)
            q = torch.einsum("srj,sj->sr", Z * Z, w[:, cls[cell]])
            out[cell] = (q * q).sum(1) * (train[cell // C] != 0)
        return out
    P = default_parts(n, n_cells) if parts is None else int(parts)
    p = native.ptr
    step = max_splits()
    for s0 in range(0, S, step):
        Sc = min(step, S - s0)
        tr, mc, wc = train[:, s0:s0 + Sc].contiguous(), mean[s0:s0 + Sc], w[s0:s0 + Sc]
        part = torch.empty((n_cells, P, Sc), dtype=torch.float64, device=dev)
        res = torch.empty((n_cells, Sc), dtype=torch.float64, device=dev)
        a = native.LdaStatArgs(X=p(X), ld=X.stride(0) if n else d, n=n, d=d, perm=p(perm), cell_off=p(cell_off),
                               n_cells=n_cells, C=C, train=p(tr), S=Sc, mean=p(mc), w=p(wc), parts=P, part=p(part),
                               out=p(res))
        _check(int(native.hip_lib().dml_lda_lw_stat(ctypes.byref(a), native.stream_handle(dev))), "lda lw_stat")
        out[:, s0:s0 + Sc] = res
    return out


def score_torch(X: torch.Tensor, rows: torch.Tensor, off, W: torch.Tensor, b: torch.Tensor):
    """(pred [NC, total] int32, dec [NC, total, C]) in float64 torch; W [S, C, NC, d], b [S, C, NC]."""
    preds, decs = [], []
    for s in range(W.shape[0]):
        Xt = X[rows[off[s]:off[s + 1]].long()].double()
        dec = torch.einsum("rj,ckj->krc", Xt, W[s]) + b[s].t().unsqueeze(1)
        decs.append(dec)
        preds.append(dec.argmax(-1).to(torch.int32))
    return torch.cat(preds, 1), torch.cat(decs, 1)


def score(X: torch.Tensor, rows: torch.Tensor, row_off, W: torch.Tensor, b: torch.Tensor,
          want_dec: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(pred int32 [NC, total], dec float64 [NC, total, C] or None) for the held-out rows
    ``rows[row_off[s]:row_off[s + 1]]`` of every split s: ``dec[k, r, c] = W[s, c, k] . x_r + b[s, c, k]``,
    pred its argmax over c (the lower class on a tie).  ``row_off`` is a host sequence; W [S, C, NC, d],
    b [S, C, NC].  More candidates than one launch takes are scored in several launches."""
    dev = X.device
    n, d = int(X.shape[0]), int(X.shape[1])
    X = X.contiguous()
    if X.dtype != torch.float32:
        raise ValueError("score: X must be float32")
    off = [int(v) for v in row_off]
    S, C, NC = int(W.shape[0]), int(W.shape[1]), int(W.shape[2])
    W = W.to(device=dev, dtype=torch.float64)
    b = b.to(device=dev, dtype=torch.float64)
    rows = rows.to(device=dev, dtype=torch.int32).contiguous()
    total = int(rows.shape[0])
    if (W.shape != (S, C, NC, d) or b.shape != (S, C, NC) or NC < 1 or len(off) != S + 1 or off[0] != 0
            or off[-1] != total or any(hi < lo for lo, hi in zip(off, off[1:]))):
        raise ValueError("score: W [S, C, NC, d], b [S, C, NC] and row_off [S + 1] over rows expected")
    if not X.is_cuda:
        pred, dec = score_torch(X, rows, off, W, b)
        return pred, (dec if want_dec else None)
    off_t = torch.tensor(off, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    pred = torch.zeros((NC, total), dtype=torch.int32, device=dev)
    dec = torch.zeros((NC, total, C), dtype=torch.float64, device=dev) if want_dec else None
    p = native.ptr
    step = max_candidates()
    for k0 in range(0, NC, step):
        nc = min(step, NC - k0)
        ncp = 1 << (nc - 1).bit_length()
        Wp = torch.zeros((S, C, ncp, d), dtype=torch.float64, device=dev)
        bp = torch.zeros((S, C, ncp), dtype=torch.float64, device=dev)
        Wp[:, :, :nc] = W[:, :, k0:k0 + nc]
        bp[:, :, :nc] = b[:, :, k0:k0 + nc]
        a = native.LdaScoreArgs(X=p(X), ld=X.stride(0) if n else d, n=n, d=d, rows=p(rows), row_off=p(off_t), S=S,
                                max_rows=max([hi - lo for lo, hi in zip(off, off[1:])], default=0), total_rows=total,
                                C=C, NC=nc, NCp=ncp, W=p(Wp), b=p(bp), pred=p(pred[k0:k0 + nc]),
                                dec=p(dec[k0:k0 + nc]) if want_dec else 0)
        _check(int(native.hip_lib().dml_lda_score(ctypes.byref(a), native.stream_handle(dev))), "lda score")
    return pred, dec

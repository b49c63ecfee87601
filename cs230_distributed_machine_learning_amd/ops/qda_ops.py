"""QuadraticDiscriminantAnalysis kernels over torch tensors on either device (docs/QDA.md).

``class_moments`` and ``score`` run csrc/kernels/qda.hip (``dml_qda_class_moments``,
``dml_qda_score``) on GPU tensors and the host twin csrc/runtime/qda_cpu.cpp on CPU tensors; the
twin is the kernels' reference, not a data path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from ..utils import native

MAX_PARTS = 16


class QdaTooLarge(RuntimeError):
    """``d`` or the candidate count is above the kernel's limit; nothing was launched."""


def max_d() -> int:
    return int(native.hip_lib().dml_qda_max_d())


def max_candidates() -> int:
    return int(native.hip_lib().dml_qda_max_candidates())


def _check(rc: int, what: str) -> None:
    if rc == native.QDA_TOO_LARGE:
        raise QdaTooLarge(f"{what}: d or the candidate count is above the kernel's limit")
    if rc:
        raise (ValueError if rc == 2 else RuntimeError)(f"{what} failed ({rc})")


def default_parts(n: int, n_cells: int) -> int:
    """Row partitions per cell: about 256 rows each at an even spread, at most MAX_PARTS."""
    return max(1, min(MAX_PARTS, -(-int(n) // (256 * max(1, int(n_cells))))))


def class_moments(X: torch.Tensor, shift: torch.Tensor, perm: torch.Tensor, cell_off: torch.Tensor,
                  parts: Optional[int] = None) -> torch.Tensor:
    """[n_cells, d + 1, d + 1] float64: per cell the moments sum z z^T of z = [x - shift, 1] over
    rows ``perm[cell_off[c]:cell_off[c + 1]]`` (entry [d, d] the count, [:d, d] the shifted column
    sums).  ``X`` float32 [n, d]; ``perm`` int32; ``cell_off`` int64 [n_cells + 1]."""
    dev = X.device
    n, d = int(X.shape[0]), int(X.shape[1])
    X = X.contiguous()
    if X.dtype != torch.float32:
        raise ValueError("class_moments: X must be float32")
    shift = shift.to(device=dev, dtype=torch.float64).contiguous()
    perm = perm.to(device=dev, dtype=torch.int32).contiguous()
    cell_off = cell_off.to(device=dev, dtype=torch.int64).contiguous()
    n_cells = int(cell_off.shape[0]) - 1
    if shift.shape != (d,) or perm.shape != (n,) or n_cells < 0:
        raise ValueError("class_moments: shift [d], perm [n] and cell_off [n_cells + 1] expected")
    P = default_parts(n, n_cells) if parts is None else int(parts)
    Dp = (d + 1 + 15) // 16 * 16
    out = torch.empty((n_cells, Dp, Dp), dtype=torch.float64, device=dev)
    part = torch.empty((n_cells, P, Dp, Dp) if X.is_cuda else (0,), dtype=torch.float64, device=dev)
    p = native.ptr
    a = native.QdaMomArgs(X=p(X), ld=X.stride(0) if n else d, n=n, d=d, shift=p(shift), perm=p(perm),
                          cell_off=p(cell_off), n_cells=n_cells, parts=P, part=p(part), out=p(out))
    if X.is_cuda:
        rc = native.hip_lib().dml_qda_class_moments(ctypes.byref(a), native.stream_handle(dev))
    else:
        rc = native.cpu_lib().dml_cpu_qda_class_moments(ctypes.byref(a))
    _check(int(rc), "qda class_moments")
    up = torch.triu(out)
    return (up + torch.triu(out, 1).transpose(1, 2))[:, :d + 1, :d + 1]


def score(X: torch.Tensor, rows: torch.Tensor, row_off, mu: torch.Tensor, V: torch.Tensor, inv: torch.Tensor,
          cst: torch.Tensor, want_dec: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(pred int32 [NC, total], dec float64 [NC, total, C] or None) for the held-out rows
    ``rows[row_off[s]:row_off[s + 1]]`` of every split s: ``dec = cst - 0.5 sum_j inv_j z_j^2``,
    ``z = (x - mu) V``.  ``row_off`` is a host sequence; mu [S, C, d], V [S, C, d, d],
    inv [S, NC, C, d], cst [S, NC, C]."""
    dev = X.device
    n, d = int(X.shape[0]), int(X.shape[1])
    X = X.contiguous()
    if X.dtype != torch.float32:
        raise ValueError("score: X must be float32")
    off = [int(v) for v in row_off]
    S, C, NC = int(mu.shape[0]), int(mu.shape[1]), int(inv.shape[1])
    f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
    mu, V, inv, cst = f64(mu), f64(V), f64(inv), f64(cst)
    rows = rows.to(device=dev, dtype=torch.int32).contiguous()
    total = int(rows.shape[0])
    if (mu.shape != (S, C, d) or V.shape != (S, C, d, d) or inv.shape != (S, NC, C, d) or cst.shape != (S, NC, C)
            or len(off) != S + 1 or off[0] != 0 or off[-1] != total or any(b < a_ for a_, b in zip(off, off[1:]))):
        raise ValueError("score: mu [S, C, d], V [S, C, d, d], inv [S, NC, C, d], cst [S, NC, C] and row_off "
                         "[S + 1] over rows expected")
    off_t = torch.tensor(off, dtype=torch.int64)
    if X.is_cuda:
        off_t = off_t.pin_memory().to(dev, non_blocking=True)
    pred = torch.zeros((NC, total), dtype=torch.int32, device=dev)
    dec = torch.zeros((NC, total, C), dtype=torch.float64, device=dev) if want_dec else None
    p = native.ptr
    a = native.QdaScoreArgs(X=p(X), ld=X.stride(0) if n else d, n=n, d=d, rows=p(rows), row_off=p(off_t), S=S,
                            max_rows=max([b - a_ for a_, b in zip(off, off[1:])], default=0), total_rows=total, C=C,
                            NC=NC, mu=p(mu), V=p(V), inv=p(inv), cst=p(cst), pred=p(pred), dec=p(dec))
    if X.is_cuda:
        rc = native.hip_lib().dml_qda_score(ctypes.byref(a), native.stream_handle(dev))
    else:
        rc = native.cpu_lib().dml_cpu_qda_score(ctypes.byref(a))
    _check(int(rc), "qda score")
    return pred, dec

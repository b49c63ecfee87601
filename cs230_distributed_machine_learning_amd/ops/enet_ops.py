"""Batched Gram coordinate descent (Lasso / ElasticNet) over torch tensors on either device.

``enet_cd`` solves F problems that share G Gram matrices: on a GPU tensor with the HIP kernel
(csrc/kernels/enet.hip ``dml_enet_cd``, one wave per problem), on a CPU tensor with its host
twin (csrc/runtime/enet_cpu.cpp ``dml_cpu_enet_cd``).  Both are sklearn's
``enet_coordinate_descent_gram`` and give the same bits (docs/ELASTIC_NET.md).
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import torch

from ..utils import native


class EnetTooLarge(RuntimeError):
    """``d`` is above the kernel's limit (``max_d()``); nothing was launched."""


def max_d() -> int:
    """The largest number of features the kernel solves (H and w of one problem in LDS)."""
    return int(native.hip_lib().dml_enet_max_d())


def problems_per_block(d: int) -> int:
    return int(native.hip_lib().dml_enet_problems_per_block(int(d)))


def _args(Q, q, ynorm2, gram_id, l1, l2, positive, max_iter, tol):
    dev = Q.device
    G, d = int(Q.shape[0]), int(Q.shape[1])
    if Q.shape != (G, d, d) or q.shape != (G, d) or ynorm2.shape != (G,):
        raise ValueError("enet_cd: Q [G, d, d], q [G, d] and ynorm2 [G] expected")
    f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    ins = [f64(Q), f64(q), f64(ynorm2), i32(gram_id), f64(l1), f64(l2), i32(positive), i32(max_iter), f64(tol)]
    F = int(ins[3].shape[0])
    if any(t.shape != (F,) for t in ins[3:]):
        raise ValueError("enet_cd: the per-problem arguments must all have shape [F]")
    outs = [torch.zeros((F, d), dtype=torch.float64, device=dev), torch.zeros(F, dtype=torch.float64, device=dev),
            torch.zeros(F, dtype=torch.float64, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)]
    p = native.ptr
    a = native.EnetArgs(Q=p(ins[0]), q=p(ins[1]), ynorm2=p(ins[2]), gram_id=p(ins[3]), l1=p(ins[4]), l2=p(ins[5]),
                        positive=p(ins[6]), max_iter=p(ins[7]), tol=p(ins[8]), w=p(outs[0]), gap=p(outs[1]),
                        tol_eff=p(outs[2]), n_iter=p(outs[3]), F=F, d=d, G=G)
    return a, ins, outs


def enet_cd_rc(Q, q, ynorm2, gram_id, l1, l2, positive, max_iter, tol, prefetch: bool = True):
    """The entry point's return code and the (w, gap, tol_eff, n_iter) buffers it was given.
    ``prefetch=False`` (GPU only) launches the kernel variant that reads every Gram row where it
    is used (``dml_enet_cd_plain``): the same bits, the baseline of scripts/bench_enet.py."""
    a, ins, outs = _args(Q, q, ynorm2, gram_id, l1, l2, positive, max_iter, tol)
    if Q.is_cuda:
        lib = native.hip_lib()
        rc = (lib.dml_enet_cd if prefetch else lib.dml_enet_cd_plain)(ctypes.byref(a), native.stream_handle(Q.device))
    else:
        if ins[3].numel() and (int(ins[3].min()) < 0 or int(ins[3].max()) >= a.G):
            raise ValueError("enet_cd: gram_id out of range")
        rc = native.cpu_lib().dml_cpu_enet_cd(ctypes.byref(a))
    del ins   # inputs stay alive until the (stream-ordered) launch was issued; torch frees in stream order
    return int(rc), tuple(outs)


def enet_cd(Q: torch.Tensor, q: torch.Tensor, ynorm2: torch.Tensor, gram_id: torch.Tensor, l1: torch.Tensor,
            l2: torch.Tensor, positive: torch.Tensor, max_iter: torch.Tensor, tol: torch.Tensor,
            prefetch: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(w [F, d], gap [F], tol_eff [F], n_iter [F] int32) of
    ``min 0.5 w^T Q w - q^T w + l1 |w|_1 + 0.5 l2 |w|^2`` for every problem f on Gram
    ``gram_id[f]``; ``l1 = alpha * l1_ratio * n``, ``l2 = alpha * (1 - l1_ratio) * n``.  The
    per-problem arguments may live on the host; they are moved next to ``Q``."""
    rc, outs = enet_cd_rc(Q, q, ynorm2, gram_id, l1, l2, positive, max_iter, tol, prefetch)
    if rc == native.ENET_D_TOO_LARGE:
        raise EnetTooLarge(f"enet_cd: d = {Q.shape[1]} is above the kernel's limit {max_d()}")
    if rc:
        raise RuntimeError(f"enet_cd failed ({rc})")
    return outs

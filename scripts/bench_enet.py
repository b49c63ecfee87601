"""Measure the Lasso / ElasticNet solve of a grid search on one GPU (docs/ELASTIC_NET.md).

The synthetic regression table of data/synthetic.py, 5 CV splits plus the holdout (6 Grams), and
for every split 50 alphas log-spaced over 4 decades below the split's
``alpha_max = max|X^T y| / n`` x l1_ratio {1, 0.5}: 600 problems at the default ``tol`` and
``max_iter``.  Reported, each as the median of ``--repeats`` timed runs after a warm-up:

  (a) the kernel (``dml_enet_cd``), device events, and (a') the same without the register
      prefetch of the Gram rows (``dml_enet_cd_plain``);
  (b) the host twin on the host's threads, including the read-back of the Grams, host clock;
  (c) the moments pass (``dml_split_moments``, all 6 splits), device events;
  (d) for context, ONE ``sklearn.linear_model.Lasso`` fit on split 0's training rows on the host.

The kernel's and the twin's results are compared bit for bit.  One JSON line per figure.

Usage: python scripts/bench_enet.py --n 1000000 --d 100 [--repeats 5] [--no-sklearn]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cs230_distributed_machine_learning_amd.data import synthetic  # noqa: E402
from cs230_distributed_machine_learning_amd.data.device import DeviceData  # noqa: E402
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, prepare_splits  # noqa: E402
from cs230_distributed_machine_learning_amd.models.linear import PenalizedLinearFamily  # noqa: E402
from cs230_distributed_machine_learning_amd.ops import enet_ops  # noqa: E402


def device_ms(fn, repeats):
    fn()   # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def host_ms(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def report(name, times, **extra):
    print(json.dumps({"figure": name, "median_ms": round(statistics.median(times), 3),
                      "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "runs": len(times), **extra}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enet.py needs a GPU")
    dev = torch.device("cuda:0")
    blocks = -(-args.n // synthetic.BLOCK)
    X, y = synthetic.make_block_range(0, blocks, args.d, informative=10, noise=1.0, seed=3, device=dev, regression=True)
    X, y = X[:args.n].contiguous(), y[:args.n].contiguous()
    dd = DeviceData(X, y, False, dev)
    prepare_splits(dd, JobSpec("Lasso", [{}], cv=5, holdout=True))
    splits = list(range(len(dd.split_names)))
    fam = PenalizedLinearFamily()
    print(json.dumps({"n": args.n, "d": args.d, "splits": dd.split_names, "omp_threads": os.environ.get("OMP_NUM_THREADS"),
                      "kernel_max_d": enet_ops.max_d(), "problems_per_block": enet_ops.problems_per_block(args.d)}),
          flush=True)

    # (c) the moments pass
    report("c_moments_pass", device_ms(lambda: fam._moments(dd, splits), args.repeats))
    M, shift = fam._moments(dd, splits)
    keys = [(s, True) for s in splits]
    A, b, yy, _xm, _ym, _live = fam._grams(M, shift, args.d, keys, splits)
    n_tr = [float(dd.train_counts[s]) for s in splits]
    amax = (b.abs().amax(1).cpu().numpy() / np.asarray(n_tr))           # per split, Lasso's alpha_max
    gid, l1, l2 = [], [], []
    for g, s in enumerate(splits):
        for ratio in (1.0, 0.5):
            for alpha in amax[g] / ratio * np.logspace(-4, -0.02, 50):
                gid.append(g)
                l1.append(alpha * ratio * n_tr[g])
                l2.append(alpha * (1.0 - ratio) * n_tr[g])
    F = len(gid)
    host_args = (torch.tensor(gid, dtype=torch.int32), torch.tensor(l1, dtype=torch.float64),
                 torch.tensor(l2, dtype=torch.float64), torch.zeros(F, dtype=torch.int32),
                 torch.full((F,), 1000, dtype=torch.int32), torch.full((F,), 1e-4, dtype=torch.float64))
    dev_args = tuple(t.to(dev) for t in host_args)

    # (a) the kernel
    res = {}

    def kernel():
        res["k"] = enet_ops.enet_cd(A, b, yy, *dev_args)

    report("a_kernel", device_ms(kernel, args.repeats), problems=F)

    # (a') the same kernel without the register prefetch of the Gram rows (k_enet_cd<0>)
    def plain():
        res["p"] = enet_ops.enet_cd(A, b, yy, *dev_args, prefetch=False)

    report("a_kernel_without_row_prefetch", device_ms(plain, args.repeats), problems=F)

    # (b) the host twin, with the read-back of the Grams
    def twin():
        res["t"] = enet_ops.enet_cd(A.cpu(), b.cpu(), yy.cpu(), *host_args)

    report("b_host_twin_with_readback", host_ms(twin, args.repeats), problems=F)
    same = all(torch.equal(k.cpu().view(torch.int64) if k.dtype == torch.float64 else k.cpu(),
                           t.view(torch.int64) if t.dtype == torch.float64 else t) for k, t in zip(res["k"], res["t"]))
    same = same and all(torch.equal(k, p_) for k, p_ in zip(res["k"], res["p"]))
    n_iter = res["t"][3]
    conv = int((res["t"][1] < res["t"][2]).sum())
    print(json.dumps({"kernel_equals_twin_bitwise": bool(same), "sweeps_total": int(n_iter.sum()),
                      "sweeps_max": int(n_iter.max()), "converged": conv, "problems": F,
                      "nonzero_coef_mean": float((res["t"][0] != 0).sum(1).double().mean())}), flush=True)

    # (d) one sklearn Lasso fit on the same rows, on the host
    if not args.no_sklearn:
        from sklearn.linear_model import Lasso

        tr = dd.train_rows[0].long()
        Xh, yh = X[tr].double().cpu().numpy(), y[tr].double().cpu().numpy()
        alpha = float(amax[0] * 1e-2)
        t0 = time.perf_counter()
        m = Lasso(alpha=alpha).fit(Xh, yh)
        report("d_sklearn_one_lasso_fit", [(time.perf_counter() - t0) * 1e3], alpha=alpha, n_iter=int(m.n_iter_))


if __name__ == "__main__":
    main()

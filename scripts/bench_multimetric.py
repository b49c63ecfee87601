"""Scoring a batch of fits under four metrics: one statistics launch against the per-fit loop
(docs/MULTIMETRIC.md).

The shape is the headline grid's scoring step: ``--fits`` fits (256 candidates x 5 folds), each
with ``--rows`` held-out rows of a 5-fold split of a (5 x rows)-row binary target, predictions
int32 class ids (80 % right).  Metrics: accuracy, f1_macro, balanced_accuracy, matthews_corrcoef.

  (a)  ``scoring.fit_statistics`` once over the concatenated row ids and predictions (one launch,
       one device->host read of F x 5 int64), then ``scoring.score_from_stats`` for every fit and
       metric on the host.  (a+) adds the ``torch.cat`` of the per-fit row ids and predictions,
       which the executor does to build the launch's inputs.
  (b)  the loop a job would otherwise need: for every fit, its targets gathered once
       (``y[rows]``) and ``scoring.score`` for each metric (a bincount and several device->host
       reads per metric).

Device events around each, one untimed warm-up, then the median of ``--reps``.  Also the bytes (a)'s
kernel reads (8 per entry: row id and prediction; the gathered targets hit in cache) over its
event time.  Before timing, both routes are compared: (a) runs the shared helpers on host
float64, (b) runs them on the device, where torch's reductions may round the last place differently
(``mean`` multiplies by 1 / n); the script reports the largest relative difference and fails above
1e-15.

Usage: python scripts/bench_multimetric.py [--fits 1280] [--rows 200000] [--reps 5] [--loop-fits N]
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

METRICS = ["accuracy", "f1_macro", "balanced_accuracy", "matthews_corrcoef"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fits", type=int, default=1280)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-fits", type=int, default=0,
                    help="time the per-fit loop over this many fits only and scale it to --fits (0: all)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from cs230_distributed_machine_learning_amd.search import scoring
    from cs230_distributed_machine_learning_amd.utils import native

    if not torch.cuda.is_available():
        raise SystemExit("bench_multimetric needs a GPU: a CPU run gives no time")
    native.hip_lib()
    dev = torch.device("cuda:0")
    F, m, folds = args.fits, args.rows, 5
    n = folds * m
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randint(0, 2, (n,), generator=g, device=dev, dtype=torch.int32)
    perm = torch.randperm(n, generator=g, device=dev).to(torch.int32)
    split_rows = [perm[k * m:(k + 1) * m].sort().values.contiguous() for k in range(folds)]
    fit_rows = [split_rows[f % folds] for f in range(F)]
    preds = []
    for f in range(F):
        right = torch.rand(m, generator=g, device=dev) < 0.8
        yt = y[fit_rows[f].long()]
        preds.append(torch.where(right, yt, 1 - yt).contiguous())
    off = np.arange(F + 1, dtype=np.int64) * m

    def stats_route(rows_cat, pred_cat):
        st = scoring.fit_statistics(rows_cat, off, pred_cat, y, 2)
        return [[scoring.score_from_stats(nm, st[f], 2) for nm in METRICS] for f in range(F)]

    def loop_route(k):
        out = []
        for f in range(k):
            yt = y[fit_rows[f].long()]
            out.append([scoring.score(nm, yt, preds[f], 2) for nm in METRICS])
        return out

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), res

    rows_cat, pred_cat = torch.cat(fit_rows), torch.cat(preds)
    k = args.loop_fits or F
    got, ref = stats_route(rows_cat, pred_cat), loop_route(k)   # the warm-up of both, and the check
    diff = max(abs(a - b) / abs(b) for f in range(k) for a, b in zip(got[f], ref[f]))
    if not diff <= 1e-15:
        raise SystemExit(f"the two routes differ by {diff} relative")
    t_a = [timed(lambda: stats_route(rows_cat, pred_cat))[0] for _ in range(args.reps)]
    t_kernel = [timed(lambda: scoring.fit_statistics(rows_cat, off, pred_cat, y, 2))[0] for _ in range(args.reps)]
    del rows_cat, pred_cat
    t_a_cat = [timed(lambda: stats_route(torch.cat(fit_rows), torch.cat(preds)))[0] for _ in range(args.reps)]
    t_b = [timed(lambda: loop_route(k))[0] * (F / k) for _ in range(args.reps)]
    med = statistics.median
    print(json.dumps({
        "bench": "multimetric_scoring", "fits": F, "rows_per_fit": m, "metrics": METRICS, "reps": args.reps,
        "routes_max_rel_diff": diff, "loop_fits_timed": k,
        "stats_route_ms": round(med(t_a), 3), "stats_route_ms_all": [round(v, 3) for v in t_a],
        "stats_route_with_cat_ms": round(med(t_a_cat), 3),
        "fit_statistics_ms": round(med(t_kernel), 3),
        "fit_statistics_read_gb_per_s": round(8.0 * F * m / (med(t_kernel) * 1e-3) / 1e9, 1),
        "per_fit_loop_ms": round(med(t_b), 3), "per_fit_loop_ms_all": [round(v, 3) for v in t_b],
        "loop_over_stats": round(med(t_b) / med(t_a), 2),
        "loop_over_stats_with_cat": round(med(t_b) / med(t_a_cat), 2),
    }))


if __name__ == "__main__":
    main()

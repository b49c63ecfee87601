"""roc_auc and average_precision of a batch of fits: one rank-statistics call against the per-fit
loop (docs/RANK_SCORES.md).

The shape is the headline grid's scoring step: ``--fits`` fits (256 candidates x 5 folds), each
with ``--rows`` held-out rows of a 5-fold split of a (5 x rows)-row binary target, float32 scores
correlated with the label, once on a 1/50 grid (forest-like: 51 distinct values) and once
continuous.

  (a)  ``scoring.rank_statistics`` once over the concatenated row ids and scores (partition, the
       12 launches of the segmented radix sort, reduce; one device->host read), then
       ``scoring.score_from_rank_stats`` for every fit and both metrics on the host.  A second run
       with ``timings`` splits the device time into partition, sort and reduce.
  (b)  the loop a job otherwise needs: for every fit, its targets gathered once (``y[rows]``) and
       ``scoring.score`` for each metric (an argsort of doubles and several device->host reads).

Device events around each, one untimed warm-up, then the median of ``--reps``.  Before timing, both
routes are compared: roc_auc must be the same double (with ``device_division``, the form of the
division ``scoring.score`` gets from torch on device tensors, as the single-metric GPU path asks),
average_precision within 1e-12 relative.
The sort's effective bandwidth counts, per pass, the keys read twice (histogram, scatter) and
written once: 4 passes x 12 bytes per key.  ``--loop-fits N`` times (b) over N fits and scales it.

Usage: python scripts/bench_rank_scores.py [--fits 1280] [--rows 200000] [--reps 5] [--loop-fits N]
Prints one JSON line per score distribution."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

METRICS = ["roc_auc", "average_precision"]


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
        raise SystemExit("bench_rank_scores needs a GPU: a CPU run gives no time")
    lib = native.hip_lib()
    dev = torch.device("cuda:0")
    F, m, folds = args.fits, args.rows, 5
    n = folds * m
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randint(0, 2, (n,), generator=g, device=dev, dtype=torch.int32)
    perm = torch.randperm(n, generator=g, device=dev).to(torch.int32)
    split_rows = [perm[k * m:(k + 1) * m].sort().values.contiguous() for k in range(folds)]
    rows_cat = torch.cat([split_rows[f % folds] for f in range(F)])
    off = np.arange(F + 1, dtype=np.int64) * m
    med = statistics.median
    tile = int(lib.dml_rank_stats_tile())
    workspace = 2 * 4 * F * m + int(lib.dml_seg_sort_hist_bytes(2 * F, m)) + 8 * F * ((m + tile - 1) // tile) + \
        8 * (4 * F + F)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), res

    for dist in ("grid", "continuous"):
        s_cat = torch.empty(F * m, dtype=torch.float32, device=dev)
        for f in range(F):   # per fit: its own draw, correlated with the label
            yt = y[rows_cat[f * m:(f + 1) * m].long()].float()
            if dist == "grid":
                s_cat[f * m:(f + 1) * m] = (torch.randint(0, 41, (m,), generator=g, device=dev).float() + 10 * yt) / 50
            else:
                s_cat[f * m:(f + 1) * m] = torch.randn(m, generator=g, device=dev) + 0.8 * yt

        def stats_route(timings=None):
            st = scoring.rank_statistics(rows_cat, off, s_cat, y, 2, pos0=1, want=scoring.WANT_AP, timings=timings)
            return [[scoring.score_from_rank_stats(nm, st[f], 2, device_division=True) for nm in METRICS]
                    for f in range(F)]

        def loop_route(k):
            out = []
            for f in range(k):
                yt = y[rows_cat[f * m:(f + 1) * m].long()]
                sf = s_cat[f * m:(f + 1) * m]
                out.append([scoring.score(nm, yt, yt, 2, None, decision=sf) for nm in METRICS])
            return out

        k = args.loop_fits or F
        got, ref = stats_route(), loop_route(k)   # the warm-up of both, and the check
        auc_equal = all(got[f][0] == ref[f][0] for f in range(k))
        ap_diff = max(abs(got[f][1] - ref[f][1]) / abs(ref[f][1]) for f in range(k))
        if not auc_equal or not ap_diff <= 1e-12:
            raise SystemExit(f"the two routes differ: roc_auc equal {auc_equal}, average_precision {ap_diff} relative")
        t_a = [timed(stats_route)[0] for _ in range(args.reps)]
        t_call = [timed(lambda: scoring.rank_statistics(rows_cat, off, s_cat, y, 2, pos0=1, want=scoring.WANT_AP))[0]
                  for _ in range(args.reps)]
        splits = []
        for _ in range(args.reps):
            tm: dict = {}
            stats_route(tm)
            splits.append(tm)
        t_b = [timed(lambda: loop_route(k))[0] * (F / k) for _ in range(args.reps)]
        sort_ms = med([tm["sort_ms"] for tm in splits])
        print(json.dumps({
            "bench": "rank_scores", "scores": dist, "fits": F, "rows_per_fit": m, "metrics": METRICS, "reps": args.reps,
            "roc_auc_equal": auc_equal, "average_precision_max_rel_diff": ap_diff, "loop_fits_timed": k,
            "stats_route_ms": round(med(t_a), 3), "stats_route_ms_all": [round(v, 3) for v in t_a],
            "rank_statistics_ms": round(med(t_call), 3),
            "partition_ms": round(med([tm["partition_ms"] for tm in splits]), 3),
            "sort_ms": round(sort_ms, 3), "sort_launches": 12,
            "reduce_ms": round(med([tm["reduce_ms"] for tm in splits]), 3),
            "sort_gb_per_s": round(4 * 12.0 * F * m / (sort_ms * 1e-3) / 1e9, 1),
            "workspace_bytes": workspace,
            "per_fit_loop_ms": round(med(t_b), 3), "per_fit_loop_ms_all": [round(v, 3) for v in t_b],
            "loop_over_stats": round(med(t_b) / med(t_a), 2),
        }), flush=True)
        del s_cat


if __name__ == "__main__":
    main()

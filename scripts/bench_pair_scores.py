"""roc_auc_ovo of a batch of multiclass fits: one pair-statistics call against the per-fit loop
(docs/RANK_SCORES.md).

``--fits`` fits, each with ``--rows`` held-out rows of a 5-fold split of a (5 x rows)-row target
with ``--classes`` classes, float32 probabilities (a softmax correlated with the label).

  (a)  ``scoring.pair_rank_statistics`` once over the concatenated row ids and probabilities (count,
       offsets, scatter, the 12 launches of the segmented radix sort, pair reduce; one device->host
       read), then ``scoring.score_from_pair_stats`` for every fit on the host.
  (b)  the loop a job needed before: for every fit, its targets gathered once (``y[rows]``) and
       ``scoring.score("roc_auc_ovo", ...)`` (two argsorts and several device->host reads per class
       pair).  ``--loop-fits N`` times it over N fits and scales it to ``--fits``.

Device events around each, a stream synchronise before and after, one untimed warm-up of both, then
``--reps`` runs alternating (a), (b); medians.  Before timing, both routes are compared: the scores
must be the same doubles (``device_division``, the form the single-metric GPU path asks for).

Usage: python scripts/bench_pair_scores.py [--fits 1280] [--rows 200000] [--classes 10] [--reps 5] [--loop-fits N]
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fits", type=int, default=1280)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-fits", type=int, default=0,
                    help="time the per-fit loop over this many fits only and scale it to --fits (0: all)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from cs230_distributed_machine_learning_amd.search import scoring
    from cs230_distributed_machine_learning_amd.utils import native

    if not torch.cuda.is_available():
        raise SystemExit("bench_pair_scores needs a GPU: a CPU run gives no time")
    native.hip_lib()
    dev = torch.device("cuda:0")
    F, m, C, folds = args.fits, args.rows, args.classes, 5
    n = folds * m
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randint(0, C, (n,), generator=g, device=dev, dtype=torch.int32)
    perm = torch.randperm(n, generator=g, device=dev).to(torch.int32)
    split_rows = [perm[k * m:(k + 1) * m].sort().values.contiguous() for k in range(folds)]
    rows_cat = torch.cat([split_rows[f % folds] for f in range(F)])
    off = np.arange(F + 1, dtype=np.int64) * m
    p_cat = torch.empty((F * m, C), dtype=torch.float32, device=dev)
    for f in range(F):   # per fit: its own draw, correlated with the label
        z = torch.randn((m, C), generator=g, device=dev)
        z.scatter_add_(1, y[rows_cat[f * m:(f + 1) * m].long()].long().view(-1, 1), torch.full((m, 1), 1.2, device=dev))
        p_cat[f * m:(f + 1) * m] = torch.softmax(z, 1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), res

    def stats_route():
        st = scoring.pair_rank_statistics(rows_cat, off, p_cat, y, C)
        return [scoring.score_from_pair_stats("roc_auc_ovo", st[f], C, device_division=True) for f in range(F)]

    k = args.loop_fits or F

    def loop_route():
        out = []
        for f in range(k):
            yt = y[rows_cat[f * m:(f + 1) * m].long()]
            out.append(scoring.score("roc_auc_ovo", yt, yt, C, p_cat[f * m:(f + 1) * m]))
        return out

    got, ref = stats_route(), loop_route()   # the warm-up of both, and the check
    equal = all(got[f] == ref[f] for f in range(k))
    if not equal:
        raise SystemExit("the two routes differ")
    t_a, t_b = [], []
    for _ in range(args.reps):   # alternating
        t_a.append(timed(stats_route)[0])
        t_b.append(timed(loop_route)[0] * (F / k))
    t_call = [timed(lambda: scoring.pair_rank_statistics(rows_cat, off, p_cat, y, C))[0] for _ in range(args.reps)]
    med = statistics.median
    print(json.dumps({
        "bench": "pair_scores", "metric": "roc_auc_ovo", "fits": F, "rows_per_fit": m, "classes": C, "reps": args.reps,
        "scores_equal": equal, "loop_fits_timed": k,
        "stats_route_ms": round(med(t_a), 3), "stats_route_ms_all": [round(v, 3) for v in t_a],
        "pair_rank_statistics_ms": round(med(t_call), 3),
        "per_fit_loop_ms": round(med(t_b), 3), "per_fit_loop_ms_all": [round(v, 3) for v in t_b],
        "loop_over_stats": round(med(t_b) / med(t_a), 2),
    }), flush=True)


if __name__ == "__main__":
    main()

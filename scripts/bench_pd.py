"""Cost of the fused partial-dependence walk against the loop it replaces.

The synthetic 1M x 100 binary table of bench.py, one RandomForestClassifier fit of 100 trees at
max_depth=None on every row, all features, grid_resolution=100 on a 50,000-row subsample (the
job's defaults).  Device-event times, median of ``--reps`` after one warm-up:

  (a)  forest_ops.partial_dependence_values for all features (a tree is walked again only where
       the baseline walk met a split on the feature and the grid point's bin leaves the interval
       that keeps every leaf of the group);
  (a') the same with every tree walked again for every grid point (``no_skip``);
  (b)  the naive loop on the first ``--naive-features`` features: for each grid point overwrite
       column f of a copy of the bins, forest_ops.predict(want_proba=True), mean; reported as
       measured and scaled to all features.

Also the host time to build and bin the grids, the share of (row, tree, feature, distinct bin)
slots that needed a second walk, and a check that (a), (a') and (b) give the same averages.

Usage: python scripts/bench_pd.py [--rows 1000000] [--features 100] [--trees 100] [--grid 100]
                                  [--max-rows 50000] [--reps 5] [--naive-features 4]
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--max-rows", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--naive-features", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    from cs230_distributed_machine_learning_amd.data import synthetic
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
    from cs230_distributed_machine_learning_amd.ops import forest_ops
    from cs230_distributed_machine_learning_amd.search.cv import ROLE_TRAIN
    from cs230_distributed_machine_learning_amd.utils import native

    native.hip_lib()
    dev = torch.device("cuda:0")
    X, y = synthetic.make_table(args.rows, args.features, informative=10, n_classes=2, noise=1.0, seed=args.seed,
                                device=dev)
    dd = DeviceData(X, y, classification=True, device=dev, name="synthetic")
    name = "RandomForestClassifier"
    params = {"n_estimators": args.trees, "max_depth": None, "min_samples_split": 2, "min_samples_leaf": 1,
              "random_state": 0}
    dd.set_splits(np.full((1, dd.n), ROLE_TRAIN, dtype=np.uint8), ["full"], key=("full",))
    fam = family_of(name)
    rp = fam.resolve(name, params, dd.train_counts[0], dd.d, dd.n_classes)
    specs = fam._specs([FitTask(0, 0, 0, name, rp)])
    Xb = dd.binned()
    T = args.trees
    fb = forest_ops.build_gpu(Xb, dd.y_cls, None, dd.roles, specs, dd.n_classes, False, fam.tiers, reuse_pool=True,
                              XbT=dd.binned_feature_major())
    torch.cuda.synchronize(dev)
    train = dd.train_rows[0]
    pick = np.sort(np.random.RandomState(0).choice(int(train.numel()), min(args.max_rows, int(train.numel())),
                                                   replace=False))
    rows = train[torch.from_numpy(pick).to(dev)]
    n = int(rows.numel())

    # the grids and their bins, as models/forest.py _attach_pd builds them (host)
    h0 = time.perf_counter()
    Xs = dd.X.index_select(0, rows.long()).t().contiguous().cpu().numpy()
    edges = dd.edges.cpu().numpy()
    feats, bins = [], []
    for f in range(dd.d):
        grid = forest_ops.partial_dependence_grid(Xs[f], args.grid, (0.05, 0.95))
        if grid is not None:
            feats.append(f)
            bins.append(forest_ops.partial_dependence_bins(grid, edges[f]))
    grid_host_ms = (time.perf_counter() - h0) * 1e3
    sub = np.zeros((len(feats), max(len(b) for b in bins)), dtype=np.uint8)
    for j, b in enumerate(bins):
        sub[j, :len(b)] = b
    ng = [len(b) for b in bins]
    distinct = [len(np.unique(b)) for b in bins]

    def timed(fn):
        """(median device-event ms over the reps after one warm-up, every rep, the last result)"""
        ms, out = [], None
        for i in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize(dev)
            if i:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), [round(v, 2) for v in ms], out

    def fused(no_skip, **kw):
        return forest_ops.partial_dependence_values(fb, Xb, 0, T, rows, feats, sub, ng, no_skip=no_skip, **kw)

    a_ms, a_all, a = timed(lambda: fused(False))
    b_ms, b_all, a_noskip = timed(lambda: fused(True))
    walked = fused(False, want_walked=True)["walked"]
    subset = list(range(min(args.naive_features, len(feats))))
    toff, roff = np.array([0, T], dtype=np.int64), np.array([0, n], dtype=np.int64)
    rows_l = rows.long()

    def naive():
        Xc = Xb.clone()
        out = np.full((len(subset), sub.shape[1]), np.nan)
        for j in subset:
            f = feats[j]
            for g in range(ng[j]):
                Xc[rows_l, f] = int(sub[j, g])
                _pred, proba = forest_ops.predict(fb, Xc, toff, roff, rows, want_proba=True)
                out[j, g] = float(proba[:, 1].double().mean())
            Xc[rows_l, f] = Xb[rows_l, f]
        return out

    n_ms, n_all, n_out = timed(naive)
    avg = a["average"][:, :, 0]
    rel = lambda p, q: float(np.nanmax(np.abs(p - q) / np.abs(q)))
    d_noskip, d_naive = rel(a_noskip["average"][:, :, 0], avg), rel(n_out, avg[subset])
    forest_ops.release_pool(fb)
    scaled = n_ms * len(feats) / max(1, len(subset))
    print(json.dumps({
        "rows": n, "features": dd.d, "features_walked": int(len(a["features"])), "trees": T, "grid": args.grid,
        "distinct_bins_mean": round(float(np.mean(distinct)), 2), "grid_host_ms": round(grid_host_ms, 1),
        "fused_ms": round(a_ms, 2), "fused_ms_all": a_all,
        "fused_no_skip_ms": round(b_ms, 2), "fused_no_skip_ms_all": b_all,
        "naive_subset": [feats[j] for j in subset], "naive_subset_ms": round(n_ms, 2), "naive_subset_ms_all": n_all,
        "naive_scaled_ms": round(scaled, 1), "naive_over_fused": round(scaled / a_ms, 2),
        "no_skip_over_fused": round(b_ms / a_ms, 3),
        "second_walk_share": round(float(walked.sum()) / (float(n) * T * float(sum(distinct))), 5),
        "max_rel_diff_no_skip": d_noskip, "max_rel_diff_naive": d_naive,
        "results_equal": bool(d_noskip <= 1e-12 and d_naive <= 1e-12),
        "baseline_mean": round(float(a["baseline"][0]), 6),
        "average_range_top5": [[int(feats[j]), round(float(np.nanmax(avg[j]) - np.nanmin(avg[j])), 5)]
                               for j in np.argsort(-(np.nanmax(avg, 1) - np.nanmin(avg, 1)))[:5]],
        "device": torch.cuda.get_device_name(dev),
    }))


if __name__ == "__main__":
    main()

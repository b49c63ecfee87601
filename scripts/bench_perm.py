"""Cost of the fused permutation-importance walk against the loop it replaces.

The synthetic 1M x 100 binary table of bench.py, a holdout split with 200,000 held-out rows, one
RandomForestClassifier fit of 100 trees at max_depth=None, K = 5 repeats.  Device-event times,
median of ``--reps`` after one warm-up:

  (a)  forest_ops.permutation_scores for all features (one launch; a tree is walked again only
       where the baseline walk met a split on the feature and the substituted bin differs);
  (a') the same with every tree walked again for every repeat (``no_skip``);
  (b)  the naive loop on the first ``--naive-features`` features some tree uses: for each (f, k)
       overwrite column f of a copy of the bins, forest_ops.predict + score_stats; reported as
       measured and scaled to all used features.

Also the share of (row, tree, feature, repeat) slots that needed a second walk, and a check that
(a), (a') and (b) give the same match counts.

Usage: python scripts/bench_perm.py [--rows 1000000] [--features 100] [--trees 100] [--repeats 5]
                                    [--reps 5] [--naive-features 4]
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--naive-features", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    from cs230_distributed_machine_learning_amd.data import synthetic
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, prepare_splits
    from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
    from cs230_distributed_machine_learning_amd.ops import forest_ops
    from cs230_distributed_machine_learning_amd.utils import native

    native.hip_lib()
    dev = torch.device("cuda:0")
    X, y = synthetic.make_table(args.rows, args.features, informative=10, n_classes=2, noise=1.0, seed=args.seed,
                                device=dev)
    dd = DeviceData(X, y, classification=True, device=dev, name="synthetic")
    name = "RandomForestClassifier"
    params = {"n_estimators": args.trees, "max_depth": None, "min_samples_split": 2, "min_samples_leaf": 1,
              "random_state": 0}
    names = prepare_splits(dd, JobSpec(name, [params], cv=0, holdout=True, random_state=0))
    hold = names.index("holdout")
    fam = family_of(name)
    rp = fam.resolve(name, params, dd.train_counts[hold], dd.d, dd.n_classes)
    specs = fam._specs([FitTask(0, 0, hold, name, rp)])
    Xb = dd.binned()
    rows = dd.test_rows[hold]
    n, T, K = int(rows.numel()), args.trees, args.repeats
    fb = forest_ops.build_gpu(Xb, dd.y_cls, None, dd.roles, specs, dd.n_classes, False, fam.tiers, reuse_pool=True,
                              XbT=dd.binned_feature_major())
    torch.cuda.synchronize(dev)
    perm = forest_ops.permutation_indices(n, K, 0)

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

    def fused(no_skip):
        return forest_ops.permutation_scores(fb, Xb, 0, T, rows, perm, ycls=dd.y_cls, no_skip=no_skip)

    a_ms, a_all, a = timed(lambda: fused(False))
    b_ms, b_all, a_noskip = timed(lambda: fused(True))
    walked = forest_ops.permutation_scores(fb, Xb, 0, T, rows, perm, ycls=dd.y_cls, want_walked=True)["walked"]
    used = [int(f) for f in a["features"]]
    subset = used[:args.naive_features]
    toff, roff = np.array([0, T], dtype=np.int64), np.array([0, n], dtype=np.int64)
    rows_l = rows.long()
    perm_dev = torch.from_numpy(perm).to(dev).long()

    def naive():
        Xc = Xb.clone()
        out = torch.zeros((len(subset), K), dtype=torch.float64)
        for j, f in enumerate(subset):
            for k in range(K):
                Xc[rows_l, f] = Xb[rows_l[perm_dev[k]], f]
                pred = forest_ops.predict(fb, Xc, toff, roff, rows)
                out[j, k] = float(forest_ops.score_stats(rows, roff, pred, ycls=dd.y_cls)[0, 0])
            Xc[rows_l, f] = Xb[rows_l, f]
        return out

    n_ms, n_all, n_out = timed(naive)
    sums = a["sums"].cpu()
    same = bool(torch.equal(sums, a_noskip["sums"].cpu())) and \
        bool(torch.equal(sums[subset].double(), n_out))
    pi = forest_ops.permutation_importance(a)
    forest_ops.release_pool(fb)
    scaled = n_ms * len(used) / max(1, len(subset))
    print(json.dumps({
        "rows_held_out": n, "features": dd.d, "features_used": len(used), "trees": T, "repeats": K,
        "fused_ms": round(a_ms, 2), "fused_ms_all": a_all,
        "fused_no_skip_ms": round(b_ms, 2), "fused_no_skip_ms_all": b_all,
        "naive_subset": subset, "naive_subset_ms": round(n_ms, 2), "naive_subset_ms_all": n_all,
        "naive_scaled_ms": round(scaled, 1), "naive_over_fused": round(scaled / a_ms, 2),
        "no_skip_over_fused": round(b_ms / a_ms, 3),
        "second_walk_share": round(float(walked.sum()) / (float(n) * T * len(used) * K), 5),
        "results_equal": same, "baseline_accuracy": round(pi["baseline_score"], 5),
        "importances_top5": [[int(i), round(float(pi["importances_mean"][i]), 5)]
                             for i in np.argsort(-pi["importances_mean"])[:5]],
        "device": torch.cuda.get_device_name(dev),
    }))


if __name__ == "__main__":
    main()

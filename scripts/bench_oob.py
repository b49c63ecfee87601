"""Cost of the out-of-bag walk and of the feature importances on the headline table.

The synthetic 1M x 100 binary table of bench.py, one RandomForestClassifier fit of 100 trees at
the headline grid's deepest setting (max_depth=None, min_samples_split=2, min_samples_leaf=1) on
a holdout split's training rows.  Device-event times, median of ``--reps`` after one warm-up:

  (a) the build (ops/forest_ops.py build_gpu);
  (b) forest_ops.predict over the training rows with that forest;
  (c) forest_ops.oob_predict over the same rows;

and, as a host clock around a synchronise, models/forest.py extract_forest (which computes the
importances) next to forest_ops.feature_importances alone on the extracted arrays.

Usage: python scripts/bench_oob.py [--rows 1000000] [--features 100] [--trees 100] [--reps 5]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch

    from cs230_distributed_machine_learning_amd.data import synthetic
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, prepare_splits
    from cs230_distributed_machine_learning_amd.models.base import FitTask, family_of
    from cs230_distributed_machine_learning_amd.models.forest import extract_forest
    from cs230_distributed_machine_learning_amd.ops import forest_ops
    from cs230_distributed_machine_learning_amd.utils import native

    native.hip_lib()
    dev = torch.device("cuda:0")
    X, y = synthetic.make_table(args.rows, args.features, informative=10, n_classes=2, noise=1.0, seed=args.seed,
                                device=dev)
    dd = DeviceData(X, y, classification=True, device=dev, name="synthetic")
    name = "RandomForestClassifier"
    params = {"n_estimators": args.trees, "max_depth": None, "min_samples_split": 2, "min_samples_leaf": 1,
              "oob_score": True, "random_state": 0}
    names = prepare_splits(dd, JobSpec(name, [params], cv=0, holdout=True, random_state=0))
    hold = names.index("holdout")
    fam = family_of(name)
    rp = fam.resolve(name, params, dd.train_counts[hold], dd.d, dd.n_classes)
    task = FitTask(0, 0, hold, name, rp)
    specs = fam._specs([task])
    Xb = dd.binned()
    rows = dd.train_rows[hold]
    n, T = int(rows.numel()), args.trees

    def timed(fn):
        """(median device-event ms over the reps after one warm-up, the last result)"""
        ms, out = [], None
        for i in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            out = fn(i == args.reps)
            e1.record()
            torch.cuda.synchronize(dev)
            if i:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), [round(v, 2) for v in ms], out

    def build(last):
        fb = forest_ops.build_gpu(Xb, dd.y_cls, None, dd.roles, specs, dd.n_classes, False, fam.tiers, reuse_pool=True,
                                  XbT=dd.binned_feature_major())
        if not last:   # the last build's pool is the forest of (b), (c) and the extraction
            torch.cuda.synchronize(dev)
            forest_ops.release_pool(fb)
        return fb

    toff, roff = np.array([0, T], dtype=np.int64), np.array([0, n], dtype=np.int64)
    build_ms, build_all, fb = timed(build)
    pred_ms, pred_all, pred = timed(lambda _l: forest_ops.predict(fb, Xb, toff, roff, rows, want_proba=True))
    oob_ms, oob_all, oob = timed(lambda _l: forest_ops.oob_predict(fb, Xb, specs, 0, T, rows))
    cnt = oob[1]
    score = forest_ops.oob_score(rows, oob[2], ycls=dd.y_cls)
    train_acc = float((pred[0] == dd.y_cls[rows.long()]).double().mean())

    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    model = extract_forest(fb, 0, T, dd, task)
    torch.cuda.synchronize(dev)
    extract_s = time.perf_counter() - t0
    nodes_dev, vals_dev = torch.from_numpy(model["nodes"]).to(dev), torch.from_numpy(model["vals"]).to(dev)
    fi_s = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fi = forest_ops.feature_importances(nodes_dev, vals_dev, T, dd.d, False, rp["criterion"])
        torch.cuda.synchronize(dev)
        fi_s.append(time.perf_counter() - t0)
    forest_ops.release_pool(fb)
    print(json.dumps({
        "rows_train": n, "features": dd.d, "trees": T, "nodes": int(model["nodes"].shape[0]),
        "build_ms": round(build_ms, 2), "build_ms_all": build_all,
        "predict_train_ms": round(pred_ms, 2), "predict_train_ms_all": pred_all,
        "oob_predict_ms": round(oob_ms, 2), "oob_predict_ms_all": oob_all,
        "oob_over_predict": round(oob_ms / pred_ms, 3),
        "oob_tree_fraction": round(float(cnt.double().mean()) / T, 4), "rows_without_oob": int((cnt == 0).sum()),
        "oob_score": round(score, 5), "train_accuracy": round(train_acc, 5),
        "extract_forest_s": round(extract_s, 3), "feature_importances_s": [round(v, 3) for v in fi_s],
        "importances_top5": [[int(i), round(float(fi[i]), 4)] for i in np.argsort(-fi)[:5]],
        "device": torch.cuda.get_device_name(dev),
    }))


if __name__ == "__main__":
    main()

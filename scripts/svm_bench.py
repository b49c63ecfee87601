#!/usr/bin/env python3
"""SVC 50k x 20, 8 candidates x cv5 on one GPU (verdict item 9): wall time of the whole
search through the engine (run_candidates), SMO iterations per problem, kernel-column
cache statistics.  ``python scripts/svm_bench.py [--rows 50000] [--cache-mb N]``.

The many-small-problems case of docs/SVM_DECISION.md is ``--rows 2000 --classes 10 --candidates 16
[--probability]``; ``--modes auto,0 --repeats R`` alternates the batched post-solve phase
(``DML_SVM_DECISION``) with the per-problem loop after one warm-up run of each, and every line
carries the post-solve wall time (from the synchronised end of the solve to the synchronised end
of the run); ``--pairs`` adds, for the batched path, the (query, support vector) pairs and FP64
operations of ``k_svm_decision`` (the count costs one host read, so time without it)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=20)
    ap.add_argument("--cv", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--probability", action="store_true")
    ap.add_argument("--candidates", type=int, default=8, choices=(8, 16))
    ap.add_argument("--modes", default="", help="comma-separated DML_SVM_DECISION values to alternate")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--pairs", action="store_true",
                    help="count the (query, support vector) pairs (DML_SVM_DECISION_PAIRS: one more host read)")
    args = ap.parse_args()
    from sklearn.datasets import make_classification

    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
    from cs230_distributed_machine_learning_amd.models.base import family_of
    from cs230_distributed_machine_learning_amd.search.grid import ParameterGrid

    X, y = make_classification(args.rows, args.features, n_informative=10, flip_y=0.05, random_state=0,
                               n_classes=args.classes, n_clusters_per_class=2 if args.classes == 2 else 1)
    dev = "cpu" if args.cpu else "cuda:0"
    dd = DeviceData(X.astype(np.float32), y, True, dev)
    Cs = [0.1, 1.0, 10.0, 100.0] if args.candidates == 8 else [0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0]
    grid = list(ParameterGrid({"C": Cs, "gamma": ["scale", "auto"]}))
    if args.probability:
        grid = [dict(p, probability=True, random_state=0) for p in grid]
    spec = JobSpec("SVC", grid, cv=args.cv, holdout=False, keep_models="none",
                   scoring="neg_log_loss" if args.probability else "accuracy")
    fam = family_of("SVC")
    sync = (lambda: None) if dev == "cpu" else torch.cuda.synchronize
    solve, marks = fam._solve, {}

    def timed_solve(*a, **k):
        solve(*a, **k)
        sync()
        marks["solved"] = time.perf_counter()

    fam._solve = timed_solve
    if args.pairs:
        os.environ["DML_SVM_DECISION_PAIRS"] = "1"
    modes = [m for m in args.modes.split(",") if m] or [os.environ.get("DML_SVM_DECISION", "auto")]
    for rep in range(-1, args.repeats):          # repeat -1 warms every mode up and is not printed
        for mode in modes:
            os.environ["DML_SVM_DECISION"] = mode
            sync()
            t0 = time.perf_counter()
            res = run_candidates(dd, spec, range(len(grid)))
            sync()
            t1 = time.perf_counter()
            if rep < 0 and (args.modes or args.repeats > 1):
                continue
            line = {"mode": mode, "rows": args.rows, "features": args.features, "classes": args.classes,
                    "candidates": len(grid), "cv": args.cv, "probability": args.probability,
                    "fits": len(grid) * args.cv, "seconds": round(t1 - t0, 3),
                    "post_solve_seconds": round(t1 - marks["solved"], 4), "ok": sum(r.ok for r in res),
                    "mean_cv": [round(r.result["mean_cv_score"], 4) for r in res],
                    "decision": getattr(fam, "last_decision_stats", None),
                    "solver": getattr(fam, "last_solve_stats", None)}
            if line["decision"].get("pairs") is not None:
                # per (query, support vector) pair: 2 d accumulate operations and the kernel function
                # (counted as one), then the multiply-add into the running sum
                line["decision"]["fp64_ops"] = line["decision"]["pairs"] * (2 * args.features + 3)
            print(json.dumps(line), flush=True)
        if not args.modes and args.repeats == 1:
            break


if __name__ == "__main__":
    main()

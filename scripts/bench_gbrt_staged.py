"""Cost of ``train_params["staged_scores"]`` on BASELINE config 6 (docs/GBRT_STAGED.md).

Config 6 of scripts/bench_configs.py -- GradientBoostingClassifier, n_estimators {100, 200} x
max_depth {3, 5}, cv=5, no holdout, the synthetic 1M x 100 binary table -- with the option off
and on, ``--reps`` alternating runs each after one untimed warm-up job: CV fits per second, the
option's cost as a percentage and as milliseconds per stage of the stage loop.

Then the stage-statistics launch alone (csrc/kernels/gbrt.hip k_gb_stage_stats +
k_gb_stage_stats_reduce) for 20 fits over the table's rows, device-event times: the bytes it
reads per second (K * 8 bytes of raw score, 4 of the class id and 2 mask bytes per row and fit).

Usage: python scripts/bench_gbrt_staged.py [--rows 1000000] [--reps 3] [--kernel-reps 20]
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--estimators", default="100,200")
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench_configs
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
    from cs230_distributed_machine_learning_amd.ops import gbrt_ops
    from cs230_distributed_machine_learning_amd.search.grid import expand_candidates
    from cs230_distributed_machine_learning_amd.utils import native

    native.hip_lib()
    dev = torch.device("cuda:0")
    dd = bench_configs._synthetic(args.rows, args.features, dev)
    dd.binned()
    ests = [int(v) for v in args.estimators.split(",")]
    cands = expand_candidates("GridSearchCV", {"param_grid": {"n_estimators": ests, "max_depth": [3, 5]}})
    model = "GradientBoostingClassifier"
    ids = list(range(len(cands)))

    def job(staged, cs=cands):
        spec = JobSpec(model, cs, cv=5, holdout=False, keep_models="none", staged={"scoring": "accuracy"} if staged else None)
        torch.cuda.synchronize(dev)
        t0 = time.time()
        res = run_candidates(dd, spec, list(range(len(cs))))
        torch.cuda.synchronize(dev)
        dt = time.time() - t0
        assert all(r.ok for r in res), [r.error for r in res if not r.ok]
        return dt, res

    warm = [dict(c, n_estimators=3) for c in cands if c["n_estimators"] == min(ests)]
    job(False, warm)
    job(True, warm)
    off, on, last = [], [], None
    for _ in range(args.reps):
        off.append(job(False)[0])
        dt, last = job(True)
        on.append(dt)
    fits = 5 * len(ids)
    loop_stages = max(ests)                       # stage-loop iterations of the job (every fit in lock-step)
    m_off, m_on = statistics.median(off), statistics.median(on)
    curve = last[0].result["staged_scores"]
    for r in last:   # the curve's last stage is the model the candidate was scored with
        assert abs(r.result["staged_scores"]["mean_cv_score"][-1] - r.result["mean_cv_score"]) < 1e-12, r.result["parameters"]

    # the statistics launch alone: 20 binary fits over the table's rows
    F, n = 20, dd.n
    g = torch.Generator(device=dev).manual_seed(1)
    raw = torch.randn((F, 1, n), dtype=torch.float64, device=dev, generator=g)
    inbag = torch.ones((F, n), dtype=torch.uint8, device=dev)
    roles = dd.roles.contiguous()
    y = dd.y_cls.to(torch.int32).contiguous()
    z = np.arange(F)
    plan = gbrt_ops.stats_plan(z, [gbrt_ops.LOSS_LOG] * F, z % int(roles.shape[0]), z, [-1] * F, z, z, [0.9] * F, K=1,
                               raw_rows=F, role_rows=int(roles.shape[0]), inbag_rows=F, val_rows=0, stat_fits=F,
                               delta_len=F, device=dev)
    stats = gbrt_ops.new_stats(F, 2, dev)
    part = torch.empty(gbrt_ops.part_words(n, F), dtype=torch.int64, device=dev)
    ms = []
    for i in range(args.kernel_reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        gbrt_ops.stage_stats(raw, y, roles, inbag, None, plan, None, stats, 1, part)
        e1.record()
        torch.cuda.synchronize(dev)
        if i:
            ms.append(e0.elapsed_time(e1))
    k_ms = statistics.median(ms)
    bytes_read = F * n * (8 + 4 + 2)
    print(json.dumps({
        "rows": n, "features": dd.d, "grid_points": len(cands), "cv_fits": fits,
        "off_s": [round(v, 3) for v in off], "on_s": [round(v, 3) for v in on],
        "off_cv_fits_per_s": round(fits / m_off, 3), "on_cv_fits_per_s": round(fits / m_on, 3),
        "on_cost_pct": round(100.0 * (m_on - m_off) / m_off, 2),
        "on_cost_ms_per_stage": round(1e3 * (m_on - m_off) / loop_stages, 3),
        "n_stages": curve["n_stages"], "best_stage": curve["best_stage"],
        "best_stage_score": round(curve["best_stage_score"], 5),
        "final_mean_cv_score": round(last[0].result["mean_cv_score"], 5),
        "stats_launch_fits": F, "stats_launch_ms": round(k_ms, 4),
        "stats_launch_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
        "stats_launch_gb_per_s": round(bytes_read / (k_ms * 1e-3) / 1e9, 1),
        "device": torch.cuda.get_device_name(dev),
    }))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Headline benchmark: CV-fits/sec (whole node), 256-pt RF GridSearchCV on 1M x 100.

BASELINE.json metric / config: RandomForestClassifier GridSearchCV, 256 grid points,
cv=5, on 1M x 100 tabular data, 1/2/4/8 MI355X (one rank per GPU, RCCL over xGMI).

* Data: synthetic 1M x 100 binary classification generated ON each GPU block-wise
  (each rank makes a contiguous row shard, then an RCCL all-gather assembles the same
  table on every rank), quantised once to uint8 bins (edges broadcast from rank 0).
* Grid (256 = 4^4): n_estimators {50,100,150,200} x max_depth {10,20,30,None} x
  min_samples_split {2,5,10,20} x min_samples_leaf {1,2,4,8}; everything else at
  sklearn defaults (gini, max_features='sqrt', bootstrap).
* Step (weak scaling): a step runs N x ``--cands-per-rank`` candidates x cv folds —
  N candidates from each cost-quantile group, so the step's cost profile is the same
  whatever N is — placed on the ranks by the engine's native LPT scheduler
  (engine/scheduler.py ``lpt_assign``) with its analytic cost model; after the fits one
  RCCL all-reduce gives every rank every candidate's CV scores (the job's result
  path).  ``value`` = total CV fits / wall seconds over exactly K timed steps (max over
  ranks).

Run: ``python bench.py [--gpus N --steps K --warmup W]`` (N>1 under torchrun, or it
re-launches itself through torch.distributed.run before touching the GPU).

A plain run sets up, warms up, times the K steps and prints the result line.
``--dump-outputs DIR`` also writes what the last timed step returned (``DIR/*.npy``) so
two builds can be compared output for output.  ``--full`` adds the secondary figures:
per-rank fit times, measured and LPT-predicted step imbalance, and the per-phase
summary on stderr.  ``--config lr`` and ``--e2e`` are other workloads with their own
result lines; they only run when asked for.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASELINE_FITS_PER_S = 0.002  # sklearn RF (100 trees) on 1M x 100, 8-core node
GRID = {
    "n_estimators": [50, 100, 150, 200],
    "max_depth": [10, 20, 30, None],
    "min_samples_split": [2, 5, 10, 20],
    "min_samples_leaf": [1, 2, 4, 8],
}


def _relaunch(args) -> int:
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(args.master_port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def _dump_outputs(out_dir: str, arrays: dict) -> None:
    """``--dump-outputs``: one ``<name>.npy`` per array, float32 / float64 only, 64 MB at most."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        total += a.nbytes
        if total > 64 * 1024 * 1024:
            raise RuntimeError(f"--dump-outputs: {name} takes the dump past 64 MB")
        np.save(os.path.join(out_dir, name + ".npy"), a)


def _result_arrays(ids, res) -> dict:
    """What ``run_candidates`` handed this rank for the candidates ``ids``: the scores only
    (its timings differ from run to run and are not outputs)."""
    import numpy as np

    return {"rank0_candidate_ids": np.asarray(ids, dtype=np.float64),
            "rank0_cv_scores": np.asarray([x.result["cv_scores"] for x in res], dtype=np.float64).reshape(len(ids), -1),
            "rank0_mean_cv_score": np.asarray([x.result["mean_cv_score"] for x in res], dtype=np.float64),
            "rank0_std_cv_score": np.asarray([x.result["std_cv_score"] for x in res], dtype=np.float64)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=("rf", "lr"), default="rf",
                    help="rf: the headline RF grid (default); lr: BASELINE config 4, RandomizedSearchCV "
                         "LogisticRegression n_iter=512 cv=5 on 10M x 1000")
    ap.add_argument("--rows", type=int, default=None, help="default 1M (rf) / 10M (lr)")
    ap.add_argument("--features", type=int, default=None, help="default 100 (rf) / 1000 (lr)")
    ap.add_argument("--cv", type=int, default=5)
    ap.add_argument("--cands-per-rank", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--master-port", type=int, default=29533)
    ap.add_argument("--cpu", action="store_true", help="run on CPU (plumbing check only)")
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--e2e", action="store_true",
                    help="the whole 256 x 5 grid as ONE J1 job through Controller + runner (LocalRunner at N=1, "
                         "the cluster DistributedRunner at N>1), incl. holdout fits and the refit")
    ap.add_argument("--chunk-target-s", type=float, default=None, help="e2e: runner slice size (estimated seconds)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the score table every "
                         "rank receives, rank 0's own results) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also report the secondary figures: per-rank fit times, measured and LPT-predicted step "
                         "imbalance, the per-phase summary on stderr (a plain run reports the headline only)")
    args = ap.parse_args()

    if args.rows is None:
        args.rows = 10_000_000 if args.config == "lr" else 1_000_000
    if args.features is None:
        args.features = 1000 if args.config == "lr" else 100
    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        return _relaunch(args)
    if args.config == "lr":
        return run_lr(args)
    if args.e2e:
        return run_e2e(args)

    import numpy as np
    import torch

    from cs230_distributed_machine_learning_amd.parallel import dist
    from cs230_distributed_machine_learning_amd.data import synthetic
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, prepare_splits, run_candidates
    from cs230_distributed_machine_learning_amd.engine.service import candidate_costs
    from cs230_distributed_machine_learning_amd.ops import binning
    from cs230_distributed_machine_learning_amd.search.grid import expand_candidates
    from cs230_distributed_machine_learning_amd.utils import trace

    inf = dist.init(want_gpu=not args.cpu)
    N, r = inf.world, inf.rank
    dev = inf.device
    if dev.type == "cuda":
        from cs230_distributed_machine_learning_amd.utils import native

        native.hip_lib()  # fail loudly if the HIP library is missing

    # ---- data: per-rank shard generated on device, RCCL all-gather -------------------------
    t_setup = time.perf_counter()
    Xs, ys = synthetic.make_table(args.rows, args.features, informative=10, n_classes=2, noise=1.0, seed=args.seed,
                                  device=dev, rank=r, world=N)
    X = dist.all_gather_rows(Xs)
    y = dist.all_gather_rows(ys)
    del Xs, ys
    dd = DeviceData(X, y, classification=True, device=dev, name="synthetic-1Mx100")
    edges = binning.quantile_edges(X) if r == 0 else torch.empty((args.features, 255), dtype=torch.float32, device=dev)
    dist.broadcast(edges, 0)
    dd._edges = edges
    dd._Xb = binning.bin_matrix(X, edges)

    cands = expand_candidates("GridSearchCV", {"param_grid": GRID})
    spec = JobSpec("RandomForestClassifier", cands, cv=args.cv, holdout=False, random_state=0, keep_models="none",
                   seed=args.seed)
    prepare_splits(dd, spec)
    if dev.type == "cuda":
        # job setup: the device arena is sized once for the largest step batch this grid
        # can form, so no timed step pays a multi-GB hipMalloc (the engine does the same
        # per job: engine/service.py)
        from cs230_distributed_machine_learning_amd.models.base import family_of

        fam = family_of(spec.model_type)
        rps = [fam.resolve(spec.model_type, p, dd.train_counts[0], dd.d, dd.n_classes) for p in cands]
        fam.presize(dd, rps, args.cands_per_rank, args.cv)
    plan = {"model_type": "RandomForestClassifier", "candidates": cands, "cv": args.cv, "holdout": False}
    costs = np.array(candidate_costs(plan, int(args.rows * (args.cv - 1) / args.cv), args.features, 2))
    order = np.argsort(-costs, kind="stable")
    c = args.cands_per_rank
    groups = np.array_split(order, c)   # cost-quantile groups; a step takes N candidates from each
    # Within a group, successive picks u = 0, 1, 2, ... visit positions in golden-ratio
    # (low-discrepancy) order: any window of steps samples the group's cost range evenly
    # (taking positions 0, 1, 2, ... would always pick each group's most expensive
    # candidates first), and len(g) consecutive picks visit every candidate once, so
    # ``--steps`` x N x c = 256 covers the whole grid exactly.
    golden = [np.argsort(np.argsort(np.mod(np.arange(len(g)) * 0.6180339887498949, 1.0), kind="stable"),
                         kind="stable") for g in groups]

    from cs230_distributed_machine_learning_amd.engine.scheduler import lpt_assign

    def step_pool(step: int):
        return [int(g[gp[(step * N + j) % len(g)]]) for g, gp in zip(groups, golden) for j in range(N)]

    def rank_step_cands(step: int):
        # the step's pool: N candidates from every cost-quantile group (N x c candidates,
        # N x c x cv fits), placed on the ranks by the native LPT scheduler with the same
        # analytic cost model the engine uses, so the slowest rank (which sets the step
        # time) is as close to the mean as the pool allows.  N=1: the rank takes the pool.
        pool = step_pool(step)
        if N == 1:
            return pool
        owner = lpt_assign([float(costs[i]) for i in pool], N)
        return [cid for cid, o in zip(pool, owner) if int(o) == r]

    dist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    setup_s = time.perf_counter() - t_setup

    score_buf = torch.zeros((N * c, args.cv), dtype=torch.float32, device=dev)
    busy: dict = {}          # timed step -> this rank's own fit seconds (before the collective)
    lpt_imb: dict = {}       # timed step -> LPT-predicted max / mean rank cost of the step's pool

    def step(s: int):
        mine = rank_step_cands(s)
        if N > 1 and args.full:
            pool = step_pool(s)
            owner = lpt_assign([float(costs[i]) for i in pool], N)
            per = np.zeros(N)
            for cid, o in zip(pool, owner):
                per[int(o)] += costs[cid]
            lpt_imb[s] = float(per.max() / max(per.mean(), 1e-12))
        t_s = time.perf_counter()
        with trace.range("step"):
            res = run_candidates(dd, spec, mine)
        busy[s] = time.perf_counter() - t_s   # results are on the host: the fits are done
        bad = [x.error for x in res if not x.ok]
        if bad:
            raise RuntimeError(f"rank {r}: failed fits: {bad[:2]}")
        # the job's result path: each rank fills its candidates' rows of the step's score
        # table, one RCCL all-reduce gives every rank every candidate's CV scores
        pos = {cid: i for i, cid in enumerate(step_pool(s))}
        score_buf.zero_()
        rows = torch.tensor([pos[cid] for cid in mine], dtype=torch.long, device=dev)
        score_buf[rows] = torch.tensor([x.result["cv_scores"] for x in res], dtype=torch.float32, device=dev)
        dist.all_reduce_sum(score_buf)
        return res

    for s in range(args.warmup):
        step(s)
    dist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    last = None
    for s in range(args.warmup, args.warmup + args.steps):
        last = step(s)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    dist.barrier()
    elapsed = time.perf_counter() - t0
    el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    dist.all_reduce_max(el)
    elapsed = float(el.item())

    fits_per_step = N * c * args.cv
    value = args.steps * fits_per_step / elapsed
    # per-rank step times (N > 1 diagnosis: a poor curve says whether the placement or the
    # ranks' speed is to blame)
    timed = list(range(args.warmup, args.warmup + args.steps))
    if args.full:
        bt = torch.tensor([busy.get(s, 0.0) for s in timed], dtype=torch.float64, device=dev)
        all_bt = dist.all_gather_rows(bt.view(1, -1)).cpu().numpy()          # [N, steps]
    if r == 0:
        if args.dump_outputs and last is not None:
            # the last timed step's result path: the score table (row i = candidate_ids[i]) as
            # every rank holds it after the all-reduce, and rank 0's own run_candidates results
            _dump_outputs(args.dump_outputs, {"candidate_ids": np.asarray(step_pool(timed[-1]), dtype=np.float64),
                                              "cv_scores": score_buf.cpu().numpy(),
                                              **_result_arrays(rank_step_cands(timed[-1]), last)})
        mean_cv = float(score_buf.mean().item())
        out = {
            "metric": "CV-fits/sec (whole node), 256-pt RF GridSearchCV on 1M×100 tabular",
            "value": round(value, 4),
            "unit": "CV-fits/s",
            "n_gpus": N,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / args.steps, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / BASELINE_FITS_PER_S, 1),
            "dtype": "fp32",
            "data": f"synthetic ({args.rows}x{args.features}, 10 informative, label noise; generated on-device, "
                    f"RCCL all-gathered; random-init forests)",
            "config": {
                "model": "RandomForestClassifier",
                "global_batch": fits_per_step,
                "seq_len": None,
                "parallelism": f"task{N}" if N > 1 else "task1",
                "rows": args.rows, "features": args.features, "grid_points": len(cands), "cv": args.cv,
                "cands_per_rank_step": c, "grid": {k: [str(v) for v in vs] for k, vs in GRID.items()},
            },
            "setup_s": round(setup_s, 2),
            "mean_cv_accuracy_last_step": round(mean_cv, 4),
            "device": str(torch.cuda.get_device_name(dev)) if dev.type == "cuda" else "cpu",
        }
        if args.full:
            out.update({
                "per_rank_fit_ms_per_step": {"min": round(1000 * float(all_bt.mean(1).min()), 1),
                                             "mean": round(1000 * float(all_bt.mean(1).mean()), 1),
                                             "max": round(1000 * float(all_bt.mean(1).max()), 1)},
                "measured_step_imbalance": round(float(np.mean(all_bt.max(0) / np.maximum(all_bt.mean(0), 1e-12))), 3),
                "lpt_predicted_imbalance": round(float(np.mean([lpt_imb[s] for s in timed])), 3) if N > 1 else 1.0,
            })
            print("phases:", json.dumps(trace.summary()), file=sys.stderr, flush=True)
        line = json.dumps(out)
        print(line, flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(line + "\n")
    dist.destroy()
    return 0


LR_DIST = {"C": {"dist": "loguniform", "a": 1e-3, "b": 1e2}, "solver": ["lbfgs", "liblinear"], "max_iter": [100]}


def run_lr(args) -> int:
    """BASELINE config 4: RandomizedSearchCV(LogisticRegression, n_iter=512, cv=5) on a
    10M x 1000 dense table (reference: per-fit sklearn lbfgs/liblinear, worker.py:39).
    Every rank holds the whole table in HBM (40 GB fp32 + the resident bf16 hi/lo MFMA
    operands); the 512 candidates are split over the ranks (task parallel) and one step
    is the whole search: each rank fits its share -- all its candidates x folds as ONE
    batched device L-BFGS over the MFMA objective (models/linear.py) -- then one RCCL
    all-reduce gives every rank every candidate's CV scores.  Total work per step is fixed
    whatever N is (strong scaling)."""
    import torch

    from cs230_distributed_machine_learning_amd.data import synthetic
    from cs230_distributed_machine_learning_amd.data.device import DeviceData
    from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, prepare_splits, run_candidates
    from cs230_distributed_machine_learning_amd.models.base import family_of
    from cs230_distributed_machine_learning_amd.parallel import dist
    from cs230_distributed_machine_learning_amd.search.grid import expand_candidates

    inf = dist.init(want_gpu=not args.cpu)
    N, r, dev = inf.world, inf.rank, inf.device
    if dev.type == "cuda":
        from cs230_distributed_machine_learning_amd.utils import native

        native.hip_lib()
    t_setup = time.perf_counter()
    Xs, ys = synthetic.make_table(args.rows, args.features, informative=10, n_classes=2, noise=1.0, seed=args.seed,
                                  device=dev, rank=r, world=N)
    X = dist.all_gather_rows(Xs)
    y = dist.all_gather_rows(ys)
    del Xs, ys
    dd = DeviceData(X, y, classification=True, device=dev, name=f"synthetic-{args.rows}x{args.features}")
    cands = expand_candidates("RandomizedSearchCV", {"param_distributions": LR_DIST, "n_iter": 512,
                                                     "random_state": 0})
    spec = JobSpec("LogisticRegression", cands, cv=args.cv, holdout=False, random_state=0, keep_models="none",
                   seed=args.seed)
    prepare_splits(dd, spec)
    mine = list(range(r, len(cands), N))
    score_buf = torch.zeros((len(cands), args.cv), dtype=torch.float32, device=dev)
    fam = family_of("LogisticRegression")
    stats = {}

    def step():
        res = run_candidates(dd, spec, mine)
        bad = [x.error for x in res if not x.ok]
        if bad:
            raise RuntimeError(f"rank {r}: failed fits: {bad[:2]}")
        score_buf.zero_()
        score_buf[torch.tensor(mine, dtype=torch.long, device=dev)] = torch.tensor(
            [x.result["cv_scores"] for x in res], dtype=torch.float32, device=dev)
        dist.all_reduce_sum(score_buf)
        stats.update(getattr(fam, "last_solve_stats", {}) or {})
        return res

    dist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    setup_s = time.perf_counter() - t_setup
    for _ in range(args.warmup):
        step()
    dist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = step()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    dist.all_reduce_max(el)
    elapsed = float(el.item())
    fits = len(cands) * args.cv
    value = args.steps * fits / elapsed
    if r == 0:
        if args.dump_outputs and last is not None:
            import numpy as np

            _dump_outputs(args.dump_outputs, {"candidate_ids": np.arange(len(cands), dtype=np.float64),
                                              "cv_scores": score_buf.cpu().numpy(), **_result_arrays(mine, last)})
        if args.full:
            from cs230_distributed_machine_learning_amd.utils import trace

            print("phases:", json.dumps(trace.summary()), file=sys.stderr, flush=True)
            print("solve:", json.dumps(stats), file=sys.stderr, flush=True)
        line = {
            "metric": "CV-fits/sec (whole node), RandomizedSearchCV LogisticRegression n_iter=512 cv=5 on 10M×1000",
            "value": round(value, 4), "unit": "CV-fits/s", "n_gpus": N, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1000.0 * elapsed / max(1, args.steps), 2), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "fp32 (bf16x3 MFMA objective)",
            "data": f"synthetic ({args.rows}x{args.features}, 10 informative; generated on-device, RCCL all-gathered)",
            "config": {"model": "LogisticRegression", "global_batch": fits, "seq_len": None,
                       "parallelism": f"task{N}", "rows": args.rows, "features": args.features,
                       "candidates": len(cands), "cv": args.cv, "search": "RandomizedSearchCV",
                       "distributions": LR_DIST},
            "setup_s": round(setup_s, 2), "best_mean_cv": round(float(score_buf.mean(1).max().item()), 4),
            "solver_stats_rank0_last_batch": stats,
            "device": str(torch.cuda.get_device_name(dev)) if dev.type == "cuda" else "cpu",
        }
        print(json.dumps(line), flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                f.write(json.dumps(line) + "\n")
    dist.destroy()
    return 0


def run_e2e(args) -> int:
    """End-to-end job path: the 256-point grid as one GridSearchCV job (J1) submitted to the
    Controller, exactly what ``MLTaskManager.train`` does (reference flow
    DistributedLibrary/src/distributed_ml/core.py:152-174 -> aws-prod/master/master.py:170-206):
    job expansion, slicing, runner dispatch, per-slice results, holdout fit per candidate
    (reference worker.py:315), best-candidate refit and model store.  The dataset goes
    through the registry; its first load (parse, H2D / RCCL broadcast, binning) is timed
    separately by a one-candidate warm-up job on the same table."""
    import tempfile
    import threading

    import torch

    from cs230_distributed_machine_learning_amd.config import Config
    from cs230_distributed_machine_learning_amd.engine.service import Controller

    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist_mode = world > 1 or os.environ.get("DML_FORCE_PG") == "1"
    cfg_kw = {}
    if args.chunk_target_s is not None:
        cfg_kw["chunk_target_s"] = args.chunk_target_s
    root = tempfile.mkdtemp(prefix="dml_e2e_")
    dev = "cpu" if args.cpu else "cuda:0"
    out: dict = {}

    def drive(ctl):
        sid = ctl.create_session()[1]["session_id"]
        # the bench's own generator (data/synthetic.py), so the e2e job fits the same table
        spec = f"classification?n={args.rows}&d={args.features}&informative=10&noise=1.0&seed={args.seed}&gen=blocks"
        t0 = time.perf_counter()
        st, msg = ctl.download_data(sid, {"dataset_url": spec, "dataset_name": "synth", "dataset_type": "synthetic"})
        assert st == 200, msg
        t_reg = time.perf_counter() - t0

        def job(jid, grid):
            return {"job_id": jid, "dataset_id": "synth", "train_params": {"target_column": "target", "test_size": 0.2},
                    "model_details": {"model_type": "RandomForestClassifier", "search_type": "GridSearchCV",
                                      "hyperparameters": {"base_estimator_params": {}, "search_params": {"param_grid": grid},
                                                          "cv_params": {"cv": args.cv}}}}

        t1 = time.perf_counter()
        st, ack = ctl.train(sid, job("warm", {"n_estimators": [4], "max_depth": [4]}))
        assert st in (200, 202), ack
        ctl.table.wait_finished(ack["job_id"], timeout=3600)
        t_load = time.perf_counter() - t1
        t2 = time.perf_counter()
        st, ack = ctl.train(sid, job("grid", GRID))
        assert st in (200, 202), ack
        ctl.table.wait_finished(ack["job_id"], timeout=7200)
        wall = time.perf_counter() - t2
        t_end = time.time()
        status = ctl.check_status(sid, ack["job_id"])[1]
        metrics = ctl.metrics(sid, ack["job_id"])[1]
        from datetime import datetime

        def _ts(x):
            return datetime.fromisoformat(x.replace("Z", "").replace("+00:00", "") + "+00:00").timestamp()

        last_slice_end = max(_ts(m["finished_at"]) for m in metrics if m.get("finished_at"))
        out["tail_s"] = t_end - last_slice_end   # refit of the best candidate + model store + publish
        # slice-level accounting: device time inside slices vs the job's wall time
        sl = {}
        for m in metrics:
            key = (m.get("worker_id"), m.get("started_at"))
            sl[key] = (m.get("slice_wall_seconds") or 0.0, m.get("slice_fits") or 0)
        out["slice_wall_sum_s"] = sum(w for w, _ in sl.values())
        out["fits_per_slice_mean"] = sum(f for _, f in sl.values()) / max(1, len(sl))
        out.update(status=status, wall=wall, t_reg=t_reg, t_load=t_load, workers=sorted({m["worker_id"] for m in metrics}),
                   last=last_slice_end, slices=len({(m.get("worker_id"), m.get("started_at")) for m in metrics}))

    if dist_mode:
        from cs230_distributed_machine_learning_amd.parallel import dist
        from cs230_distributed_machine_learning_amd.parallel.runner import DistributedRunner, WorkerCore, worker_loop

        inf = dist.init(want_gpu=not args.cpu)
        core = WorkerCore(inf.device)
        if inf.rank != 0:
            worker_loop(core)
            dist.destroy()
            return 0
        runner = DistributedRunner(core)
        ctl = Controller(Config(data_root=root, device=str(inf.device), **cfg_kw), runner=runner)
        err = []

        def th():
            try:
                drive(ctl)
            except Exception as e:  # pragma: no cover
                err.append(e)
            finally:
                runner.shutdown()

        t = threading.Thread(target=th, daemon=True)
        t.start()
        runner.serve_forever()
        t.join()
        if err:
            raise err[0]
        runner_name = f"distributed x{inf.world}"
    else:
        ctl = Controller(Config(data_root=root, device=dev, **cfg_kw))
        drive(ctl)
        ctl.shutdown()
        runner_name = "local"
    status = out["status"]
    assert status["job_status"] == "completed", status
    res = status["job_result"]["results"]
    n_cv = sum(len(r.get("cv_scores", [])) for r in res)
    n_all = sum(int(r.get("n_fits", 0)) for r in res)
    value = n_cv / out["wall"]
    line = {
        "metric": "CV-fits/sec (whole node), 256-pt RF GridSearchCV on 1M×100 tabular", "mode": "e2e-job",
        "value": round(value, 4), "unit": "CV-fits/s", "n_gpus": world, "steps": 1, "warmup": 1,
        "ms_per_step": round(1000 * out["wall"], 1), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": round(value / BASELINE_FITS_PER_S, 1), "dtype": "fp32",
        "data": f"synthetic ({args.rows}x{args.features}) registered through the dataset registry",
        "config": {"model": "RandomForestClassifier", "global_batch": n_cv, "seq_len": None,
                   "parallelism": runner_name, "grid_points": len(res), "cv": args.cv},
        "all_fits_incl_holdout": n_all, "all_fits_per_s": round(n_all / out["wall"], 4),
        "job_wall_s": round(out["wall"], 2), "dataset_register_s": round(out["t_reg"], 2),
        "dataset_first_load_s": round(out["t_load"], 2), "workers": out["workers"],
        "best_mean_cv": round(status["best_result"]["mean_cv_score"], 4),
        "best_model_stored": bool(status["best_result"].get("model_path")),
        "refit_and_publish_s": round(out["tail_s"], 2),
        "slices": out["slices"], "fits_per_slice_mean": round(out["fits_per_slice_mean"], 1),
        "slice_wall_sum_s": round(out["slice_wall_sum_s"], 2),
    }
    if args.dump_outputs:
        import numpy as np

        _dump_outputs(args.dump_outputs, {
            "cv_scores": np.asarray([r.get("cv_scores", []) for r in res], dtype=np.float64),
            "mean_cv_score": np.asarray([r.get("mean_cv_score", math.nan) for r in res], dtype=np.float64)})
    if args.full:
        from cs230_distributed_machine_learning_amd.utils import trace

        print("phases:", json.dumps(trace.summary()), file=sys.stderr, flush=True)
    print(json.dumps(line), flush=True)
    if args.json_out:
        with open(args.json_out, "w") as f:
            f.write(json.dumps(line) + "\n")
    if dist_mode:
        from cs230_distributed_machine_learning_amd.parallel import dist

        dist.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())

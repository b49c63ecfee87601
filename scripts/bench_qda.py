"""QuadraticDiscriminantAnalysis search timing (docs/QDA.md): 8 reg_param values x cv5 on a
200,000 x 64 table with 10 classes, the HIP path against the float64 torch path
(``DML_QDA_KERNEL=0``) in the same process, alternating, after a warm-up run of each.
Prints one JSON line (seconds per search; medians of 7)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cs230_distributed_machine_learning_amd.data.device import DeviceData  # noqa: E402
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates  # noqa: E402

rng = np.random.default_rng(0)
n, d, C = 200_000, 64, 10
y = rng.integers(0, C, n)
X = rng.normal(size=(n, d)).astype(np.float32) + (0.3 * y[:, None]).astype(np.float32)
dd = DeviceData(X, y, True, "cuda")
grid = [{"reg_param": r} for r in np.linspace(0.0, 0.7, 8).tolist()]


def once(kernel: bool):
    os.environ["DML_QDA_KERNEL"] = "1" if kernel else "0"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run_candidates(dd, JobSpec("QuadraticDiscriminantAnalysis", grid, cv=5, holdout=False), range(8))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(r.ok for r in res)
    return dt, [r.result["mean_cv_score"] for r in res]


for k in (True, False):
    once(k)
times = {True: [], False: []}
scores = {}
for _rep in range(7):
    for k in (True, False):
        dt, scores[k] = once(k)
        times[k].append(dt)
print(json.dumps({"hip_s": times[True], "torch_s": times[False], "hip_median": float(np.median(times[True])),
                  "torch_median": float(np.median(times[False])), "scores_equal": scores[True] == scores[False]}))

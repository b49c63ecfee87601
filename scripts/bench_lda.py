"""LinearDiscriminantAnalysis search timing (docs/LDA.md): 8 candidates (five float shrinkages,
``"auto"`` under lsqr and eigen, and svd) x cv5 on a 200,000 x 64 table with 10 classes, the HIP
path against the float64 torch path (``DML_LDA_KERNEL=0``) in the same process, alternating, after
a warm-up run of each; where sklearn imports, its ``GridSearchCV`` on the host as well.
Prints one JSON line (seconds per search; medians of 7, sklearn of 2)."""
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
grid = ([{"solver": "lsqr", "shrinkage": a} for a in (None, 0.01, 0.1, 0.3, 1.0)]
        + [{"solver": "lsqr", "shrinkage": "auto"}, {"solver": "eigen", "shrinkage": "auto"}, {"solver": "svd"}])


def once(kernel: bool):
    os.environ["DML_LDA_KERNEL"] = "1" if kernel else "0"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run_candidates(dd, JobSpec("LinearDiscriminantAnalysis", grid, cv=5, holdout=False), range(len(grid)))
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
out = {"hip_s": times[True], "torch_s": times[False], "hip_median": float(np.median(times[True])),
       "torch_median": float(np.median(times[False])), "scores_equal": scores[True] == scores[False]}
try:
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    from sklearn.model_selection import GridSearchCV
except ImportError:
    pass
else:
    X64, sk_s = X.astype(np.float64), []
    for _rep in range(2):
        t0 = time.perf_counter()
        ref = GridSearchCV(LinearDiscriminantAnalysis(), [{k: [v] for k, v in p.items()} for p in grid], cv=5).fit(X64, y)
        sk_s.append(time.perf_counter() - t0)
    out.update(sklearn_s=sk_s, sklearn_score_gap=float(np.abs(ref.cv_results_["mean_test_score"] - scores[True]).max()))
print(json.dumps(out))

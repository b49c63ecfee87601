"""The Gram coordinate-descent kernel (csrc/kernels/enet.hip ``dml_enet_cd``) against its host twin,
bit for bit, and the penalised linear family on a GPU table (docs/ELASTIC_NET.md).

The twin itself is checked against sklearn's solver in test_enet.py; here ``w``, ``gap`` and
``n_iter`` of the kernel must be the twin's bits:

* every case of enet_cases.py in ONE launch (432 problems on six Grams zero-padded to d = 130,
  consecutive problems on different Grams), launched twice on two streams: both equal the twin;
* every d on its own, unpadded (d = 1, 3, 63, 64, 65, 130: below, at and above one wave's lanes),
  with the cases that stop by 1000 sweeps -- the 100000-sweep cases of these Grams run in the
  launch above;
* one problem more than a workgroup holds; d at the kernel's limit; one above it, which the entry
  refuses and the family solves with the twin.
"""
import warnings

import numpy as np
import pytest
import torch

import enet_cases as ec
from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, build_tasks, prepare_splits, run_candidates
from cs230_distributed_machine_learning_amd.models import linear
from cs230_distributed_machine_learning_amd.models.base import family_of
from cs230_distributed_machine_learning_amd.ops import enet_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu
KEYS = ("Q", "q", "ynorm2", "gram_id", "l1", "l2", "positive", "max_iter", "tol")
DEV = "cuda:0"


def _solve(inp, device):
    return enet_ops.enet_cd(*[torch.from_numpy(np.array(inp[k])).to(device) for k in KEYS])


def _assert_same_bits(got, ref, what):
    for name, a, b in zip(("w", "gap", "tol_eff", "n_iter"), got, ref):
        a, b = a.cpu(), b.cpu()
        if a.dtype == torch.float64:   # compare the bit patterns: -0.0 and NaN payloads count
            a, b = a.view(torch.int64), b.view(torch.int64)
        bad = (a != b).nonzero()
        assert bad.numel() == 0, f"{what}: {name} differs from the twin at {bad[:5].tolist()} ({bad.shape[0]} entries)"


@pytest.fixture(scope="module")
def batched():
    inp, ps = ec.batched_inputs()
    return inp, ps, _solve(inp, "cpu")


def test_every_case_in_one_launch_equals_the_twin_and_repeats(batched):
    inp, ps, ref = batched
    assert len(ps) == 432 and len(set(inp["gram_id"][:6].tolist())) == 6   # interleaved Grams
    assert int(ref[3].max()) == 100000 and int(ref[3].min()) == 1            # both exits are in the batch
    side = torch.cuda.Stream(DEV)   # the two launches run side by side: each uploads its own inputs
    first = _solve(inp, DEV)
    with torch.cuda.stream(side):
        second = _solve(inp, DEV)
    torch.cuda.synchronize(DEV)
    _assert_same_bits(first, ref, "all cases, one launch")
    _assert_same_bits(second, ref, "all cases, second launch")


@pytest.mark.parametrize("d", ec.DS)
def test_each_d_unpadded_equals_the_twin(d):
    inp, ps = ec.solver_inputs(d)
    keep = np.array([not (p["max_iter"] > 1000 and p["l1_ratio"] == 0.0) for p in ps])   # see the module docstring
    sub = dict(inp, **{k: inp[k][keep] for k in KEYS[3:]})
    assert keep.sum() == 64
    _assert_same_bits(_solve(sub, DEV), _solve(sub, "cpu"), f"d = {d}")


@pytest.mark.parametrize("d", [3, 130])
def test_one_problem_more_than_a_workgroup_holds(d):
    per_block = enet_ops.problems_per_block(d)
    assert per_block >= 1
    inp, ps = ec.solver_inputs(d)
    pick = [i for i, p in enumerate(ps) if p["max_iter"] == 1000 and p["l1_ratio"] > 0][:per_block + 1]
    assert len(pick) == per_block + 1
    sub = dict(inp, **{k: inp[k][pick] for k in KEYS[3:]})
    _assert_same_bits(_solve(sub, DEV), _solve(sub, "cpu"), f"{per_block + 1} problems at d = {d}")
    none = dict(inp, **{k: inp[k][:0] for k in KEYS[3:]})
    assert _solve(none, DEV)[0].shape == (0, d)            # F = 0 launches nothing


def _wide_problem(d):
    """A 48-row problem d features wide: (A [1, d, d], b [1, d], yy [1]) float64 and two problems'
    arguments -- a Lasso that keeps a few coordinates, and a positive ElasticNet cut at 5 sweeps."""
    g = torch.Generator().manual_seed(5)
    X = torch.randn((48, d), generator=g, dtype=torch.float64)
    y = X[:, 0] * 2.0 - X[:, 7] + 0.1 * torch.randn(48, generator=g, dtype=torch.float64)
    n = 48.0
    args = ([0, 0], [0.5 * n, 0.3 * n], [0.0, 0.2 * n], [0, 1], [1000, 5], [1e-4, 1e-6])
    targs = [torch.tensor(v, dtype=torch.float64 if isinstance(v[0], float) else torch.int32) for v in args]
    return (X.t() @ X)[None].contiguous(), (X.t() @ y)[None].contiguous(), (y @ y).view(1), args, targs


def test_kernel_at_the_largest_d_equals_the_twin():
    """d = the queried limit: one problem fills the workgroup's whole LDS, and the rows are read
    where they are used (no register prefetch above d = 1024).  The prefetch-free variant is
    also run at a small d, where the default launch prefetches: the same bits."""
    limit = enet_ops.max_d()
    assert limit > 1024 and enet_ops.problems_per_block(limit) == 1
    A, b, yy, _args, targs = _wide_problem(limit)
    ref = enet_ops.enet_cd(A, b, yy, *targs)
    _assert_same_bits(enet_ops.enet_cd(A.to(DEV), b.to(DEV), yy.to(DEV), *targs), ref, "d = the limit")
    assert int((ref[0] != 0).sum()) >= 2 and ref[3].tolist()[1] == 5
    inp, ps = ec.solver_inputs(130)
    keep = np.array([p["max_iter"] <= 1000 for p in ps])
    sub = dict(inp, **{k: inp[k][keep] for k in KEYS[3:]})
    plain = enet_ops.enet_cd(*[torch.from_numpy(np.array(sub[k])).to(DEV) for k in KEYS], prefetch=False)
    _assert_same_bits(plain, _solve(sub, "cpu"), "d = 130 without the prefetch")


def test_d_above_the_limit_is_refused_and_the_family_falls_back_to_the_twin(monkeypatch):
    """The limit is queried, never assumed.  One feature above it the entry point returns its
    documented code and launches nothing, and a job on a GPU table that wide runs through
    ``PenalizedLinearFamily.run`` with the host twin: the coefficients of the same job on the CPU
    data path, ``n_iter``, the warnings, predictions on the device.  The moments of this test come
    from the torch route (``host_split_moments``, device-agnostic) on both data paths: the test is
    about the solver's fallback, not about the moments kernel at that width."""
    limit = enet_ops.max_d()
    assert limit >= 130 and enet_ops.problems_per_block(limit + 1) == 0
    d = limit + 1
    A, b, yy, args, targs = _wide_problem(d)
    rc, _outs = enet_ops.enet_cd_rc(A.to(DEV), b.to(DEV), yy.to(DEV), *targs)
    assert rc == native.ENET_D_TOO_LARGE == 3
    with pytest.raises(enet_ops.EnetTooLarge):
        enet_ops.enet_cd(A.to(DEV), b.to(DEV), yy.to(DEV), *targs)
    got, solver = linear.PenalizedLinearFamily._enet(A.to(DEV), b.to(DEV), yy.to(DEV), *args)
    assert solver == "twin" and all(t.is_cuda for t in got)
    _assert_same_bits(got, enet_ops.enet_cd(A, b, yy, *targs), "d above the limit")
    # the same through run(), on a GPU table
    monkeypatch.setattr(linear.PenalizedLinearFamily, "_moments",
                        staticmethod(lambda data, splits: linear.host_split_moments(data, splits)))
    rng = np.random.RandomState(3)
    X = rng.normal(size=(96, d)).astype(np.float32)
    y = (2.0 * X[:, 0] - X[:, 7] + 0.1 * rng.normal(size=96)).astype(np.float32)
    grid = [{"alpha": 0.3}, {"alpha": 0.05, "max_iter": 2}]
    spec = JobSpec("Lasso", grid, cv=2, holdout=False, keep_models="all")
    fam = family_of("Lasso")
    runs = {}
    for dev in (DEV, "cpu"):
        dd = DeviceData(X, y, False, dev)
        prepare_splits(dd, spec)
        tasks, errors = build_tasks(dd, spec, range(2))
        assert not errors
        runs[dev] = (tasks, fam.run(dd, tasks, keep_models=True), dd)
    for (t, og), oc in zip(zip(runs[DEV][0], runs[DEV][1]), runs["cpu"][1]):
        assert og.info["solver"] == "twin" and og.pred.is_cuda and og.pred.dtype == torch.float32
        assert og.info["n_iter"] >= 1 and (t.params["max_iter"] != 2 or og.info["n_iter"] == oc.info["n_iter"] == 2)
        assert (t.params["max_iter"] == 2) == any("did not converge" in w for w in og.info["warnings"])
        scale = np.abs(oc.model["coef"]).max()
        assert scale > 0 and np.abs(og.model["coef"] - oc.model["coef"]).max() <= 1e-8 * scale
        assert np.abs(og.pred.cpu().numpy() - oc.pred.numpy()).max() <= 1e-4
    res = run_candidates(runs[DEV][2], JobSpec("Lasso", grid, cv=2, holdout=False), range(2))
    assert all(r.ok for r in res) and res[1].result["n_iter"] == [2, 2]
    assert np.isfinite(res[0].result["cv_scores"]).all()


def _job_table():
    rng = np.random.RandomState(11)
    X = rng.normal(size=(600, 12)).astype(np.float32)
    X[:, 3] += 0.6 * X[:, 0]
    coef = np.array([1.5, 0, 0, -0.8, 0, 0.4, 0, 0, 0, 0, 0.05, 0])
    y = (X.astype(np.float64) @ coef + 0.7 + 0.3 * rng.normal(size=600)).astype(np.float32)
    return X, y


def test_family_on_a_gpu_table_matches_sklearn_and_never_reads_the_moments_back():
    from sklearn.linear_model import Lasso
    from sklearn.model_selection import GridSearchCV

    X, y = _job_table()
    dd = DeviceData(X, y, False, DEV)
    alphas = [0.01, 0.1, 1.0]
    grid = [{"alpha": a, "tol": 1e-10, "max_iter": 100000} for a in alphas]
    spec = JobSpec("Lasso", grid, cv=3, holdout=True, keep_models="all")
    res = run_candidates(dd, spec, range(3))
    ref = GridSearchCV(Lasso(tol=1e-10, max_iter=100000), {"alpha": alphas}, cv=3).fit(X.astype(np.float64),
                                                                                       y.astype(np.float64))
    for r, mean in zip(res, ref.cv_results_["mean_test_score"]):
        assert r.ok, r.error
        assert abs(r.result["mean_cv_score"] - mean) <= 1e-6, (r.result["mean_cv_score"], mean)
        assert len(r.result["n_iter"]) == 3 and all(i >= 1 for i in r.result["n_iter"])
        assert np.isfinite(r.result["r2_score"]) and r.model["kind"] == "linear_regression"
    fam = linear.PenalizedLinearFamily()
    # the solve itself: Grams from the device moments, problem arguments up from pinned memory,
    # one launch -- no synchronising call (torch counts them) until the results are read
    prepare_splits(dd, spec)
    tasks, _errors = build_tasks(dd, spec, range(3))
    splits = sorted({t.split for t in tasks})
    M, shift = fam._moments(dd, splits)
    keys = sorted({(t.split, True) for t in tasks})
    n_tr = [float(dd.train_counts[t.split]) for t in tasks]
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            A, b, yy, _xm, _ym, _live = fam._grams(M, shift, dd.d, keys, splits)
            out, solver = fam._enet(A, b, yy, [keys.index((t.split, True)) for t in tasks],
                            [t.params["alpha"] * n for t, n in zip(tasks, n_tr)], [0.0] * len(tasks),
                            [0] * len(tasks), [100000] * len(tasks), [1e-10] * len(tasks))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    syncs = [str(w.message) for w in rec if "synchroniz" in str(w.message)]
    assert not syncs, syncs
    assert solver == "kernel" and out[0].is_cuda and bool((out[1] < out[2]).all())      # every fit converged

"""The fold-grouped LogisticRegression objective (models/linear.py, csrc/kernels/lr_mfma.hip).

``MfmaOperands`` permutes the operand rows so that every split's held-out rows fill whole
256-row tiles; ``MfmaPlan.layout(True)`` lays the fits out split by split; ``k_lr_fwd3`` then
skips the GEMM of (row tile, column tile) items without a training row (``ct_split`` /
``rt_skip``) and ``k_lr_grad3`` writes zero slabs for such K slices (``kskip``).  Every case
here asserts that this path is taken, and compares loss and gradient with a float64 reference
computed in plain torch in the dataset's ORIGINAL row order (so it is blind to the
permutation).  Also: the operand builder ``dml_split_hilo`` against torch's own bf16
rounding, ``fold_grouped_perm`` on the CPU, the HBM-roles branch of ``k_lr_fwd3`` (more than
8 role rows), and the skip tables combined with the stopped-fit masks and ``w_zero``.

The tolerances are the ones ``test_lr_mfma_objective_matches_fp32`` applies to this kernel at
these sizes: loss ``rtol=2e-5, atol=1e-6``; gradient ``max |dG| / max|G| per column < 2e-4``.
"""
import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.data.device import DeviceData
from cs230_distributed_machine_learning_amd.engine.executor import JobSpec, run_candidates
from cs230_distributed_machine_learning_amd.search.cv import ROLE_TEST, ROLE_TRAIN, make_split_roles

gpu = pytest.mark.gpu
DEV = "cuda:0"
LOSS_RTOL, LOSS_ATOL, GRAD_TOL = 2e-5, 1e-6, 2e-4


def _dd(X, y, clf, dev, cv=5, holdout=True):
    dd = DeviceData(X, y, clf, dev)
    roles, names = make_split_roles(np.asarray(y), cv, clf, holdout=holdout, test_size=0.2, random_state=0)
    dd.set_splits(roles, names)
    return dd


def _lr_batch(dd, specs):
    from cs230_distributed_machine_learning_amd.models import linear
    from cs230_distributed_machine_learning_amd.models.base import FitTask

    fam = linear.LogisticFamily()
    tasks = []
    for i, (params, split) in enumerate(specs):
        rp = fam.resolve("LogisticRegression", params, dd.n, dd.d, dd.n_classes)
        tasks.append(FitTask(task_id=i, candidate=i, split=split, model_type="LogisticRegression", params=rp))
    return fam, linear._Batch(dd, tasks)


# name -> dataset / batch ("data": cases sharing one dataset and reference), plan settings and
# what the plan must look like.  Uneven fit counts per split: padding columns sit in the middle
# of the batch and a split's last column tile is part padding.
CASES = {
    # (a) binary, cv=5 + holdout: plain layout 1504 -> 1536 columns, by split 1529 -> 1536
    "a": dict(data="a", classes=2, n=5003, d=130, cv=5, holdout=True, per_split=[250, 256, 243, 256, 250, 249],
              by_split=True, holdout_skipped=False),
    # (b) the same over row chunks of 512 rows (row_base / bk_off / per-chunk kskip)
    "b": dict(data="a", classes=2, n=5003, d=130, cv=5, holdout=True, per_split=[250, 256, 243, 256, 250, 249],
              by_split=True, holdout_skipped=False, rt_gb="0.004"),
    # (c) config 4's structure at 580 rows per fold; and with a holdout split that is skipped too
    # (test rows of the holdout in runs of ~520 rows per fold)
    "c": dict(data="c", classes=2, n=2900, d=40, cv=5, holdout=False, per_split=[256] * 5, by_split=True),
    "c_holdout": dict(data="c_holdout", classes=2, n=13001, d=33, cv=5, holdout=True, per_split=[256] * 6,
                      by_split=True, holdout_skipped=True),
    # (d) three classes: 42 fits per 128-column tile, 252 columns per split, softmax / OvR alternating
    "d": dict(data="d", classes=3, n=5003, d=64, cv=5, holdout=True, per_split=[84] * 6, by_split=True,
              holdout_skipped=False),
    # (e) ten role rows: roles read from HBM (role_at), together with the skip
    "e": dict(data="e", classes=2, n=5003, d=70, cv=10, holdout=False, per_split=[250] * 10, by_split=True),
    # (f) ten role rows, too few fits for the by-split layout (300 -> 512 columns against 2560)
    "f": dict(data="f", classes=2, n=5003, d=70, cv=10, holdout=False, per_split=[30] * 10, by_split=False),
}


class _Data:
    """One dataset + batch + weights and the float64 reference of its objective (built once)."""


_BUILT = {}


def _reference(dd, b, W):
    """Data terms of the objective in float64, plain torch, original row order."""
    from cs230_distributed_machine_learning_amd.models import linear

    d = dd.d
    X = dd.X.double()
    Z = X @ W[:d].double() + (W[d] * b.icpt_col).double()
    R, loss = linear.link_grad_torch(Z, dd.y_cls, dd.roles, b.col0_l, b.K_l, b.kind_l, b.split_l, b.scale.tolist(),
                                     b.cw)
    G = torch.empty(W.shape, dtype=torch.float64, device=W.device)
    G[:d] = X.t() @ R
    G[d] = R.sum(0) * b.icpt_col
    return loss, G


def _data(key):
    if key in _BUILT:
        return _BUILT[key]
    c = CASES[key]
    assert c["data"] == key
    n, d, C = c["n"], c["d"], c["classes"]
    rng = np.random.RandomState(1000 + 7 * C + d)
    X = (rng.randn(n, d) * rng.uniform(0.1, 3.0, d)).astype(np.float32)
    y = rng.randint(0, C, n)
    dd = _dd(X, y, True, DEV, cv=c["cv"], holdout=c["holdout"])
    assert len(dd.split_names) == len(c["per_split"])
    specs, i = [], 0
    for s, cnt in enumerate(c["per_split"]):
        for _ in range(cnt):   # lbfgs (softmax) / liblinear (OvR) alternating, every fifth fit class-weighted
            p = {"C": float(10.0 ** rng.uniform(-2, 2)), "solver": ["lbfgs", "liblinear"][i % 2]}
            if i % 5 == 0:
                p["class_weight"] = "balanced"
            specs.append((p, s))
            i += 1
    specs = [specs[j] for j in rng.permutation(len(specs))]   # batch order mixes the splits
    o = _Data()
    o.dd = dd
    o.fam, o.b = _lr_batch(dd, specs)
    o.W = torch.randn((d + 1, o.b.M), device=DEV, generator=torch.Generator(DEV).manual_seed(d)) * 0.05
    o.f_ref, o.G_ref = _reference(dd, o.b, o.W)
    _BUILT[key] = o
    return o


def _plan(name, monkeypatch):
    """A fresh MfmaPlan of the case on its (shared) dataset; asserts the path the case is for."""
    from cs230_distributed_machine_learning_amd.models import linear

    c = CASES[name]
    o = _data(c["data"])
    if c.get("rt_gb") is not None:
        monkeypatch.setenv("DML_LR_RT_GB", c["rt_gb"])
    mf = linear.MfmaPlan(o.dd, o.b)
    assert mf.v3
    assert mf.by_split == c["by_split"]
    assert (mf.n_chunks > 1) == (c.get("rt_gb") is not None)
    if c["cv"] + c["holdout"] > 8:
        assert int(mf.fwd_l[0].n_splits) > 8          # k_lr_fwd3's V3_ROLE_ROWS: roles not staged in LDS
    if c["by_split"]:
        assert mf.ops.perm is not None
        assert int(mf.ops.rt_skip.sum()) > 0
        assert all(fa.ct_split != 0 and fa.rt_skip != 0 for fa in mf.fwd_l)
        assert all(ga.kskip != 0 for ga in mf.grad_l)
        if c["holdout"]:
            # n = 5003: the holdout's test rows lie in five runs of ~200 rows, none fills a row tile
            # of data rows (the ragged last tile, test rows + padding, is not counted here);
            # n = 13001: runs of ~520 rows do
            full = o.dd.n // linear._ROW_TILE
            assert bool(mf.ops.rt_skip[-1, :full].any()) == c["holdout_skipped"]
    else:
        assert mf.kskip_l is None and all(fa.ct_split == 0 for fa in mf.fwd_l)
    return o, mf


def _rel_errors(f, G, f_ref, G_ref):
    """(max relative loss error, max |dG| over the column's max |G|)."""
    le = float(((f.double() - f_ref).abs() / f_ref.abs().clamp_min(1e-300)).max())
    ge = float(((G.double() - G_ref).abs() / G_ref.abs().amax(0, keepdim=True).clamp_min(1e-6)).max())
    return le, ge


def _assert_close(f, G, f_ref, G_ref):
    torch.testing.assert_close(f.double(), f_ref.double(), rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert _rel_errors(f, G, f_ref, G_ref)[1] < GRAD_TOL


def _check_skip_tables(o, mf):
    """The tables against the roles themselves: a skipped row tile / gradient slice holds no
    training row of the split, and only tiles whose fits all belong to that split are labelled."""
    from cs230_distributed_machine_learning_amd.models import linear

    b, ops = o.b, mf.ops
    perm = ops.perm.cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(o.dd.n))
    roles = o.dd.roles.cpu().numpy()
    assert np.array_equal(ops.roles.cpu().numpy(), roles[:, perm])
    assert np.array_equal(ops.y.cpu().numpy(), o.dd.y_cls.cpu().numpy()[perm])
    S = roles.shape[0]
    train = np.zeros((S, ops.npad), dtype=bool)
    train[:, :o.dd.n] = roles[:, perm] == ROLE_TRAIN
    rt = ops.rt_skip.cpu().numpy()
    assert rt.shape == (S, ops.npad // linear._ROW_TILE)
    assert np.array_equal(rt != 0, ~train.reshape(S, -1, linear._ROW_TILE).any(2))
    # splits of the fits of every column tile / m tile, from the fits' own first columns
    col0 = mf.fit_col0.cpu().numpy()
    ct_sets = [set() for _ in range(mf.Mp // linear._TILE)]
    for f in range(b.F):
        for ct in {col0[f] // linear._TILE, (col0[f] + b.K_l[f] - 1) // linear._TILE}:
            ct_sets[ct].add(b.split_l[f])
    cts = mf.ct_split.cpu().numpy()
    for ct, ss in enumerate(ct_sets):
        assert cts[ct] == (next(iter(ss)) if len(ss) == 1 else -1)
    assert (cts >= 0).sum() >= S                      # every split labels a column tile of its own
    flagged = zero_in_single = 0
    for ci, (ks_t, ga) in enumerate(zip(mf.kskip_l, mf.grad_l)):
        ks = ks_t.cpu().numpy()
        m_tiles, Sl, Kc, rows_c, r0 = int(ga.m_tiles), int(ga.S), int(ga.Kc), int(ga.Kp), int(ga.bk_off)
        assert ks.shape == (m_tiles, Sl) and int(ga.slab0) == ci * Sl
        for mt in range(m_tiles):
            ss = ct_sets[2 * mt] | ct_sets[2 * mt + 1]
            for k in range(Sl):
                a0, a1 = r0 + k * Kc, r0 + min((k + 1) * Kc, rows_c)
                if a1 <= a0:                          # slice past the chunk's rows: no work either way
                    continue
                if ks[mt, k]:
                    assert len(ss) == 1 and not train[next(iter(ss)), a0:a1].any()
                    flagged += 1
                elif len(ss) == 1:
                    assert train[next(iter(ss)), a0:a1].any()   # nothing skippable is left unskipped
                    zero_in_single += 1
    assert flagged > 0 and zero_in_single > 0


# ---- 1. fold-skip objective against float64 -----------------------------------------------------

@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fold_skip_objective_matches_float64(name, monkeypatch):
    """Loss and data gradient of the matrix-core objective against the float64 reference, on plans
    that skip held-out row tiles and gradient slices (cases a-e) and on the HBM-roles branch
    without the by-split layout (f).  The fp32 path's error against the same reference is printed
    next to it (``-s`` shows both).  Measured on an MI355X over the seven cases: matrix-core path
    loss 3.8e-7 .. 6.3e-7 (relative), gradient 7.6e-6 .. 8.9e-6; fp32 path loss 1e-8 .. 4.6e-8,
    gradient 2.4e-6 .. 5.9e-6 -- the bounds (2e-5, 2e-4) leave the MFMA path a factor of ~20."""
    o, mf = _plan(name, monkeypatch)
    b, dd, W = o.b, o.dd, o.W
    f1, G1 = mf.objective(dd, b, W)
    assert b.mf is None
    # fp32 path (library GEMMs + link kernel); it adds the penalty, so does its reference
    f0, G0 = o.fam._objective(dd, b, W)
    torch.cuda.synchronize()
    reg = W.double() * b.lam_col.double()
    reg[dd.d] = reg[dd.d] * b.pen_icpt_col.double()
    pen = 0.5 * torch.zeros(b.F, dtype=torch.float64, device=DEV).index_add_(0, b.col_fit, (W.double() * reg).sum(0))
    e_mf = _rel_errors(f1, G1, o.f_ref, o.G_ref)
    e_32 = _rel_errors(f0, G0, o.f_ref + pen, o.G_ref + reg)
    print(f"\n[fold-skip {name}] mfma: loss {e_mf[0]:.3e} grad {e_mf[1]:.3e} | "
          f"fp32: loss {e_32[0]:.3e} grad {e_32[1]:.3e} | cols {mf.Mp} chunks {mf.n_chunks} "
          f"rt_skip {int(mf.ops.rt_skip.sum()) if mf.ops.rt_skip is not None else 0}")
    assert bool(torch.isfinite(G1).all())
    _assert_close(f1, G1, o.f_ref, o.G_ref)
    if mf.by_split:
        _check_skip_tables(o, mf)


# ---- 2. the skip is exact ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_fold_skip_is_exact(name, monkeypatch):
    """A skipped tile contributes exact zeros: the same plan and permutation evaluated with
    the skip tables switched off gives the same bits (loss, gradient, per-tile loss partials).
    And the unpermuted layout (DML_LR_FOLD_ROWS=0) agrees at the kernel's tolerances."""
    from cs230_distributed_machine_learning_amd.models import linear

    o, mf = _plan(name, monkeypatch)
    b, dd, W = o.b, o.dd, o.W
    f1, G1 = mf.objective(dd, b, W)
    lp1 = mf.lpart.clone()
    for fa in mf.fwd_l:
        fa.ct_split = 0
    for ga in mf.grad_l:
        ga.kskip = 0
    f2, G2 = mf.objective(dd, b, W)
    torch.cuda.synchronize()
    assert torch.equal(f1, f2)
    assert torch.equal(G1, G2)
    assert torch.equal(lp1, mf.lpart)
    # original row order: other operands, other summation order
    fold_ops = dd._lr_mfma_ops
    monkeypatch.setenv("DML_LR_FOLD_ROWS", "0")
    dd._lr_mfma_ops = None
    try:
        plain = linear.MfmaPlan(dd, b)
        assert plain.ops is not fold_ops and plain.ops.perm is None and plain.ops.rt_skip is None
        assert plain.v3 and not plain.by_split
        f3, G3 = plain.objective(dd, b, W)
        torch.cuda.synchronize()
    finally:
        dd._lr_mfma_ops = fold_ops
    _assert_close(f1, G1, f3, G3.double())
    _assert_close(f3, G3, o.f_ref, o.G_ref)


# ---- 3. skip tables combined with stopped fits and w_zero ---------------------------------------

@gpu
def test_fold_skip_with_stopped_fits_and_w_zero(monkeypatch):
    """``live`` / ``mlive`` (stopped fits) on top of ``ct_split`` / ``kskip``: active fits keep
    their bits, a later unmasked call restores everything, and ``w_zero`` equals W = 0."""
    from cs230_distributed_machine_learning_amd.models import linear

    o, mf = _plan("a", monkeypatch)
    b, dd, W, fam = o.b, o.dd, o.W, o.fam
    b.mf = mf
    try:
        f_all, G_all = mf.objective(dd, b, W)
        # by split: 0, 1 stopped altogether (their m tiles go idle); 2 keeps only its first column
        # tile, 4 only its second; 3 keeps every other fit (both tiles half alive); 5 runs on
        ct = (mf.fit_col0.cpu().numpy() // linear._TILE) % 2
        act_l = []
        for f in range(b.F):
            s = b.split_l[f]
            act_l.append({0: False, 1: False, 2: ct[f] == 0, 3: f % 2 == 0, 4: ct[f] == 1, 5: True}[s])
        act = torch.tensor(act_l, device=DEV)
        f_act, G_act = mf.objective(dd, b, W, act)
        torch.cuda.synchronize()
        col_tiles = mf.Mp // linear._TILE
        assert int(mf.live[0]) == 6 and 0 < int(mf.live[0]) < col_tiles
        assert mf.mlive.tolist() == [0, 0, 1, 1, 1, 1]
        assert torch.equal(f_act[act], f_all[act])
        cols = act[b.col_fit]
        assert torch.equal(G_act[:, cols], G_all[:, cols])
        f_again, G_again = mf.objective(dd, b, W)        # no mask: every tile again
        assert torch.equal(f_again, f_all) and torch.equal(G_again, G_all)
        _assert_close(f_again, G_again, o.f_ref, o.G_ref)
        # the solver's first evaluation (W = 0) skips the forward GEMM: same result
        W0 = torch.zeros_like(W)
        f0, G0 = mf.objective(dd, b, W0)
        f0z, G0z = mf.objective(dd, b, W0, w_zero=True)
        assert torch.equal(f0z, f0) and torch.equal(G0z, G0)
        assert all(fa.w_zero == 1 for fa in mf.fwd_l)
        # ... and the grouped fp32 start the solver actually uses agrees with it
        fg, Gg = fam._objective_at_zero(dd, b)
        torch.cuda.synchronize()
        _assert_close(f0, G0, fg, Gg.double())
        f0r, G0r = _reference(dd, b, W0)
        _assert_close(f0, G0, f0r, G0r)
    finally:
        b.mf = None


# ---- 4. dml_split_hilo ---------------------------------------------------------------------------

def _roundup(x, m):
    return (x + m - 1) // m * m


def _hilo_case(rows, cols, ld, transpose, with_perm):
    from cs230_distributed_machine_learning_amd.utils import native

    g = torch.Generator(DEV).manual_seed(rows * 1000 + cols)
    src = torch.randn((rows, ld), device=DEV, generator=g) * torch.exp2(
        torch.randint(-6, 7, (rows, ld), device=DEV, generator=g).float())
    src.view(-1)[5::7] = 0.0                # exact zeros and exactly representable values among them
    src.view(-1)[3::11] = 1.5
    x = src[:, :cols]
    perm = torch.randperm(rows, device=DEV, generator=g) if with_perm else None
    K = _roundup(rows, 256) if transpose else _roundup(cols, 32)            # as MfmaOperands pads
    drows = _roundup(cols + 1, 128) if transpose else _roundup(rows, 256)
    hi = torch.zeros((K // 32, drows, 32), dtype=torch.bfloat16, device=DEV)
    lo = torch.zeros_like(hi)
    rc = native.hip_lib().dml_split_hilo(native.ptr(src), rows, cols, ld, native.ptr(hi), native.ptr(lo), drows,
                                         transpose, native.ptr(perm) if perm is not None else None,
                                         native.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    xp = x[perm] if perm is not None else x
    op = torch.zeros((drows, K), dtype=torch.float32, device=DEV)           # operand [rows, k], zero padded
    if transpose:
        op[:cols, :rows] = xp.t()
    else:
        op[:rows, :cols] = xp
    e_hi = op.bfloat16()
    e_lo = (op - e_hi.float()).bfloat16()
    tiled = lambda t: t.view(drows, K // 32, 32).permute(1, 0, 2).contiguous()
    assert torch.equal(hi.view(torch.int16), tiled(e_hi).view(torch.int16))   # bits: padding is +0
    assert torch.equal(lo.view(torch.int16), tiled(e_lo).view(torch.int16))
    # two roundings to 8-bit significands: |x - hi| <= 2^-9 |x|, |(x - hi) - lo| <= 2^-9 |x - hi|
    back = (hi.double() + lo.double()).permute(1, 0, 2).reshape(drows, K)
    assert bool(((op.double() - back).abs() <= 2.0 ** -16 * op.double().abs()).all())


@gpu
@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 31), (65, 33), (300, 130), (257, 64)])
def test_split_hilo_matches_torch_bf16(rows, cols, transpose, with_perm):
    """bf16 hi / lo split in the K-tiled layout ``[K/32, drows, 32]``: bit-equal to torch's
    round-to-nearest-even, every padding element zero, ragged 64 x 64 tile edges included."""
    _hilo_case(rows, cols, cols, transpose, with_perm)


@gpu
@pytest.mark.parametrize("transpose", [0, 1])
def test_split_hilo_leading_dimension(transpose):
    """Source rows wider than the columns converted (ld > cols)."""
    _hilo_case(300, 130, 137, transpose, True)


# ---- 5. fold_grouped_perm (CPU) ------------------------------------------------------------------

@pytest.mark.parametrize("cv,holdout,classes,n", [(5, True, 2, 5003), (10, False, 2, 5003), (5, True, 3, 2900)])
def test_fold_grouped_perm_is_a_stable_grouping(cv, holdout, classes, n):
    from cs230_distributed_machine_learning_amd.models import linear

    rng = np.random.RandomState(cv + classes)
    y = rng.randint(0, classes, n)
    roles, names = make_split_roles(y, cv, True, holdout=holdout, test_size=0.2, random_state=0)
    perm = linear.fold_grouped_perm(torch.from_numpy(roles)).numpy()
    assert np.array_equal(np.sort(perm), np.arange(n))                 # a permutation
    pr = roles[:, perm]
    same = (pr[:, 1:] == pr[:, :-1]).all(0)                            # neighbour has the same role tuple
    n_tuples = len(np.unique(roles, axis=1).T)
    assert int((~same).sum()) == n_tuples - 1                          # equal tuples are adjacent ...
    assert (np.diff(perm)[same] > 0).all()                             # ... and keep their original order
    assert (np.diff(perm) > 0).sum() < n - 1                           # (the order did change)
    for s in range(cv):                                                # each CV split's test rows: one run
        t = np.flatnonzero(pr[s] == ROLE_TEST)
        assert len(t) > 0 and t[-1] - t[0] + 1 == len(t)
        if holdout:                                                    # inside it: holdout train, then test
            h = pr[-1, t[0]:t[-1] + 1]
            assert (np.diff(h.astype(np.int64)) >= 0).all()


# ---- 6. end to end -------------------------------------------------------------------------------

@gpu
def test_fold_rows_search_matches_plain_rows(monkeypatch):
    """A 256-candidate search (1536 fits: cv=5 + holdout) with and without fold-grouped rows."""
    from cs230_distributed_machine_learning_amd.models import linear

    rng = np.random.RandomState(8)
    X = rng.randn(20000, 40).astype(np.float32)
    y = (X @ rng.randn(40) + 2 * rng.randn(20000) > 0).astype(int)
    grid = [{"C": float(c), "solver": ["lbfgs", "liblinear"][i % 2]} for i, c in enumerate(10.0 ** np.linspace(-3, 2, 256))]
    seen = []
    init = linear.MfmaPlan.__init__

    def recording_init(self, data, b):
        init(self, data, b)
        seen.append(self.by_split)

    monkeypatch.setattr(linear.MfmaPlan, "__init__", recording_init)
    out, used = {}, {}
    for flag in ("0", "1"):
        monkeypatch.setenv("DML_LR_FOLD_ROWS", flag)
        del seen[:]
        dd = DeviceData(X, y, True, DEV)
        res = run_candidates(dd, JobSpec("LogisticRegression", grid, cv=5), range(len(grid)))
        assert all(r.ok for r in res), [r.error for r in res]
        out[flag] = np.array([r.result["mean_cv_score"] for r in res])
        used[flag] = list(seen)
    assert used["1"] and all(used["1"])
    assert used["0"] and not any(used["0"])
    np.testing.assert_allclose(out["1"], out["0"], atol=1e-3)

"""The subtree tier's two-features-per-sort evaluation (forest.hip DML_SUB_PK16: sub_sort_pk2 /
sub_post_pk for nodes of 33..64 rows, sub_node_seg_pk<8 / 16 / 32> below) against the host
builder: node-for-node equal trees and bit-for-bit equal predictions, at the node sizes on both
sides of every path and segment-width boundary (64, 33 | 32, 17 | 16, 9 | 8, 3, 2 rows), with an
odd and an even feature count, max_features below, at and above what one pass holds, constant
columns, identical columns, weights up to 12, and the packed sort networks on their own."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

G = 64                                   # rows per group
NG = 62                                  # whole groups; the table's tail is one group of 32 rows
N = NG * G + 32
RUNS_A = (33, 17, 9, 3, 2)               # a group's rows cut into runs by COL_RUN, two patterns
RUNS_B = (32, 16, 8, 3, 3, 2)
SIZES = (64, 33, 32, 17, 16, 9, 8, 3, 2)
COL_RUN, COL_GROUP, COL_DUP_A, COL_DUP_B, COL_EQ = 2, 3, 5, 13, 7
COLS_CONST = (0, 11, 20)
TIERS = dict(sub_max=64, wave_max=255, block_max=1024, chunk=512)
TIERS_BIG = dict(sub_max=64, wave_max=256, block_max=1024, chunk=512, bigsub_max=256)


@functools.lru_cache(maxsize=None)
def _table(d):
    """Bins (drawn directly) and labels.  Groups of 64 consecutive rows, group g cut by COL_RUN into
    runs of RUNS_A (even g) or RUNS_B (odd g) rows; the label is the parity of run + group with
    the first row of every run flipped, so no run is pure.  COL_RUN is the only informative column
    inside a group and COL_GROUP between two groups: a tree over one group splits run after run
    off (inner nodes of 33, 17, 9, ... rows), a tree over two groups splits them apart first (two
    subtree roots of 64 rows handed down by the wave tier).  Three columns are constant (visiting
    positions that do not count towards max_features), two are identical (equal scores: the
    earlier visiting position must win), one has four distinct bins (equal scores between bins of
    one feature: the lowest must win).  The splits (role rows): 0 every row; 1 two groups; 2, 3
    one group of each pattern; 4.. one run of each size in SIZES (64: a third whole group)."""
    rs = np.random.RandomState(23)
    Xb = rs.randint(0, 256, size=(N, d)).astype(np.uint8)
    idx = np.arange(N)
    grp, pos = idx // G, idx % G
    run = np.zeros(N, np.int64)
    first = np.zeros(N, bool)
    starts = {}
    for g in range(NG + 1):
        cuts = np.cumsum((0,) + (RUNS_A if g % 2 == 0 else RUNS_B))
        for r in range(len(cuts) - 1):
            m = (grp == g) & (pos >= cuts[r]) & (pos < cuts[r + 1])
            run[m] = r
            first[m & (pos == cuts[r])] = True
            starts[(g, r)] = (g * G + cuts[r], cuts[r + 1] - cuts[r])
    Xb[:, COL_RUN] = 10 + 30 * run
    Xb[:, COL_GROUP] = 4 * grp
    Xb[:, COL_DUP_B] = Xb[:, COL_DUP_A]
    Xb[:, COL_EQ] = 50 * rs.randint(0, 4, size=N)
    for cc in COLS_CONST:
        Xb[:, cc] = 77
    y = ((run + grp) & 1) ^ first
    roles = [np.ones(N, np.uint8)]
    for groups in ((0, 1), (2,), (3,)):
        roles.append(np.isin(grp, groups).astype(np.uint8))
    root_rows = [N, 2 * G, G, G]
    where = {64: None, 33: (4, 0), 32: (5, 0), 17: (4, 1), 16: (5, 1), 9: (4, 2), 8: (5, 2), 3: (4, 3), 2: (4, 4)}
    for size in SIZES:
        r = np.zeros(N, np.uint8)
        if where[size] is None:
            r[grp == 6] = 1
        else:
            s0, ln = starts[where[size]]
            assert ln == size
            r[s0:s0 + ln] = 1
        roles.append(r)
        root_rows.append(size)
    return np.ascontiguousarray(Xb), y.astype(np.int32), np.stack(roles), tuple(root_rows)


def _shifted_table(kind):
    """Bootstrap tables that keep every row (weight >= 1), so a node's row count is the number
    of rows routed to it: 1 + Poisson(1), or weights uniform on 1..12 (the largest the table holds)."""
    if kind == "uniform":
        return np.array([0] + [int(j / 12.0 * 2.0**32) for j in range(1, 12)], dtype=np.uint32)
    t = native.poisson_cdf_table(1.0).astype(np.uint32)
    return np.concatenate([np.zeros(1, np.uint32), t[:-1]])


def _specs(nsplits, criterion, msl, k, bootstrap=1, per_split=4):
    """per_split trees on every split: tree 0 weighs 1 + Poisson(1), tree 1 uniformly 1..12 (both
    keep every row), the others draw a plain Poisson(1) bootstrap."""
    T = nsplits * per_split
    specs = forest_ops.make_specs(T)
    for t in range(T):
        s = specs[t]
        s["seed"] = 977 + t
        s["split"] = t // per_split
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = msl
        s["max_features"] = k
        s["bootstrap"] = bootstrap
        s["criterion"] = criterion
        s["pois_cdf"] = (_shifted_table("poisson"), _shifted_table("uniform"))[t % per_split] if t % per_split < 2 \
            else native.poisson_cdf_table(1.0)
    return specs


def _keeps_rows(specs, t, per_split=4):
    return specs[t]["bootstrap"] == 0 or t % per_split < 2


def _canon(nodes, vals, T):
    out = []
    for t in range(T):
        seq, stack = [], [t]
        while stack:
            i = stack.pop()
            s, l = int(nodes[i, 0]), int(nodes[i, 1])
            seq.append((s, tuple(np.round(vals[i], 6))))
            if s >= 0:
                stack.append(l + 1)
                stack.append(l)
        out.append(seq)
    return out


def _cpu():
    lib = native.cpu_lib()
    lib.dml_node_root_key.restype = ctypes.c_uint64
    lib.dml_node_root_key.argtypes = [ctypes.c_uint64]
    lib.dml_node_child_key.restype = ctypes.c_uint64
    lib.dml_node_child_key.argtypes = [ctypes.c_uint64, ctypes.c_int32]
    lib.dml_node_visit_order.restype = None
    lib.dml_node_visit_order.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]
    return lib


def _walk(nodes, Xb, root, rows, seed):
    """(node index, rows, node key, is root) of the split nodes of one tree that keeps every row."""
    lib = _cpu()
    stack = [(root, rows, lib.dml_node_root_key(int(seed)), True)]
    while stack:
        i, r, key, is_root = stack.pop()
        s, l = int(nodes[i, 0]), int(nodes[i, 1])
        if s < 0:
            continue
        yield i, r, key, is_root
        left = Xb[r, s // 256] <= (s % 256)
        stack.append((l, r[left], lib.dml_node_child_key(key, 0), False))
        stack.append((l + 1, r[~left], lib.dml_node_child_key(key, 1), False))


def _const_halves(Xb, rows, key, k):
    """The key halves (0: first, 1: second) in which the packed evaluation of this subtree node
    meets a table-wide constant column before max_features non-constant ones are found."""
    lib = _cpu()
    d = Xb.shape[1]
    order = np.zeros(d, np.int32)
    lib.dml_node_visit_order(key, d, order.ctypes.data)
    cnt = len(rows)
    S = 1 if cnt > 32 else 64 // (8 if cnt <= 8 else 16 if cnt <= 16 else 32)
    halves, nonconst = set(), 0
    for p, f in enumerate(order):
        if nonconst >= k:
            break
        col = Xb[rows, f]
        if col.min() != col.max():
            nonconst += 1
        elif f in COLS_CONST:
            halves.add((p // S) % 2)
    return halves


def _compare(d, specs, tiers, cw=None, expect_sizes=False, k=None):
    Xb_cpu, ycls, roles, root_rows = _table(d)
    dev = torch.device("cuda:0")
    assert native.hip_lib().dml_forest_sub_pk16() == 1          # the library under test sorts two features per pass
    Xb = torch.from_numpy(Xb_cpu).to(dev)
    T = len(specs)
    kw = {} if cw is None else {"cw": cw.copy()}
    g = forest_ops.build_gpu(Xb, torch.from_numpy(ycls).to(dev), None, torch.from_numpy(roles).to(dev), specs, 2, False,
                             forest_ops.ForestTiers(**tiers), **kw)
    c = forest_ops.build_cpu(Xb_cpu, ycls, None, roles, specs, 2, False, **kw)
    assert g.stats["tier_nodes"][0] > 0
    gc = _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), T)
    cc = _canon(c.nodes, c.vals, T)
    assert sum(map(len, gc)) == sum(map(len, cc)) == c.stats["nodes"]
    assert gc == cc
    rows = np.arange(N, dtype=np.int32)
    roff, toff = np.array([0, N]), np.array([0, T])
    pg = forest_ops.predict(g, Xb, toff, roff, torch.from_numpy(rows).to(dev)).cpu().numpy()
    pc = forest_ops.predict(c, Xb_cpu, toff, roff, rows)
    assert np.array_equal(pg, pc)
    if not expect_sizes:
        return c
    # from the host builder's trees that keep every row: the roots and the inner split nodes hold
    # exactly the sizes under test, and a constant column is met in a first key half in one tree
    # and in a second key half in another
    roots, inner, half_trees = set(), set(), {0: set(), 1: set()}
    for t in range(T):
        if not _keeps_rows(specs, t):
            continue
        sp = int(specs[t]["split"])
        tr = np.flatnonzero(roles[sp])
        assert len(tr) == root_rows[sp]
        for _, r, key, is_root in _walk(c.nodes, Xb_cpu, t, tr, specs[t]["seed"]):
            (roots if is_root else inner).add(len(r))
            if len(r) <= 64:
                for h in _const_halves(Xb_cpu, r, key, k):
                    half_trees[h].add(t)
    assert set(SIZES) <= roots, sorted(roots)
    assert set(SIZES) <= inner, sorted(inner & set(range(65)))
    assert half_trees[0] and half_trees[1] and len(half_trees[0] | half_trees[1]) > 1, half_trees
    return c


@pytest.mark.parametrize("k", [1, 5, 10, 0])          # 0: every feature
@pytest.mark.parametrize("d", [23, 24])
def test_packed_subtree_sizes_and_max_features(d, k):
    """Gini, min_samples_leaf 1: every node size under test occurs as a subtree root and as an inner
    node; max_features 1 (an odd budget the first half fills), 5, 10 and d."""
    kk = k or d
    _compare(d, _specs(13, forest_ops.GINI, 1, kk), TIERS, expect_sizes=True, k=kk)


@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
@pytest.mark.parametrize("msl", [1, 4])
def test_packed_subtree_criteria_and_leaf_sizes(criterion, msl):
    _compare(23, _specs(13, criterion, msl, 10), TIERS)


@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
def test_packed_subtree_unit_weights(criterion):
    _compare(24, _specs(13, criterion, 1, 5, bootstrap=0), TIERS)


def test_packed_subtree_uniform_weights_reach_the_table_top():
    """The trees weighted uniformly on 1..12: a 64-row root's total weight is far above its row
    count (the expected mean weight is 6.5), so the 4-bit weight field is exercised to its top."""
    specs = _specs(13, forest_ops.GINI, 1, 10)
    c = _compare(24, specs, TIERS)
    _, _, roles, root_rows = _table(24)
    seen = 0
    for t in range(len(specs)):
        sp = int(specs[t]["split"])
        if t % 4 == 1 and root_rows[sp] == 64:
            assert 5 * 64 < c.vals[t].sum() < 8 * 64
            seen += 1
    assert seen >= 3


def test_packed_subtree_class_weights():
    """class_weight (dict rows and balanced_subsample) takes the generic kernel: the packed keys
    hold the integer weights, the class weights multiply the sums at evaluation."""
    specs = _specs(13, forest_ops.GINI, 1, 10)
    T = len(specs)
    cw = np.ones((T, 2))
    for t in range(T):
        specs[t]["cw_mode"] = (0, 1, 2)[t % 3]
        if t % 3 == 1:
            cw[t] = (1.0, 3.5)
    _compare(23, specs, TIERS, cw=cw)


@pytest.mark.parametrize("criterion,msl,k,d", [(forest_ops.GINI, 1, 5, 23), (forest_ops.GINI, 4, 10, 24),
                                                (forest_ops.ENTROPY, 1, 24, 24), (forest_ops.GINI, 1, 1, 23)])
def test_packed_subtree_in_bigsub(criterion, msl, k, d):
    """k_bigsub grows its nodes of <= 64 rows with the same subtree_dfs."""
    _compare(d, _specs(13, criterion, msl, k), TIERS_BIG)


def _build_pair(Xb_cpu, ycls, yreg, roles, specs, n_classes, is_reg, **kw):
    dev = torch.device("cuda:0")
    Xb = torch.from_numpy(Xb_cpu).to(dev)
    g = forest_ops.build_gpu(Xb, None if ycls is None else torch.from_numpy(ycls).to(dev),
                             None if yreg is None else torch.from_numpy(yreg).to(dev), torch.from_numpy(roles).to(dev),
                             specs, n_classes, is_reg, forest_ops.ForestTiers(**TIERS), **kw)
    c = forest_ops.build_cpu(Xb_cpu, ycls, yreg, roles, specs, n_classes, is_reg, **kw)
    T = len(specs)
    assert g.stats["tier_nodes"][0] > 0
    assert _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), T) == _canon(c.nodes, c.vals, T)


def test_other_builds_keep_their_subtree_code():
    """Regression, three classes and monotonic_cst do not take the packed path: their subtrees
    equal the host builder's as before."""
    Xb_cpu, ycls, roles, _ = _table(23)
    rs = np.random.RandomState(5)
    specs = _specs(13, forest_ops.GINI, 1, 10)
    y3 = (ycls + 2 * (rs.rand(N) < 0.3)).astype(np.int32) % 3
    _build_pair(Xb_cpu, y3, None, roles, specs, 3, False)
    mono = np.zeros((1, 23), dtype=np.int8)
    mono[0, COL_RUN], mono[0, 4] = 1, -1
    _build_pair(Xb_cpu, ycls, None, roles, specs, 2, False, mono=mono)
    sreg = _specs(13, 2, 1, 10)                      # squared error
    yreg = (ycls + 0.25 * rs.randn(N)).astype(np.float32)
    _build_pair(Xb_cpu, None, yreg, roles, sreg, 1, True)


def _sort_inputs():
    rs = np.random.RandomState(3)
    lo, hi = [], []

    def add(a, b):
        lo.append(np.asarray(a, np.uint32))
        hi.append(np.asarray(b, np.uint32))

    for _ in range(8):
        add(rs.randint(0, 1 << 16, 64), rs.randint(0, 1 << 16, 64))            # random 16-bit values
    add(np.full(64, 7), np.full(64, 0xFFFF))                                   # all equal
    add(np.arange(64) * 9, np.arange(64)[::-1] * 11)                           # sorted / reversed: the halves disagree
    add(np.arange(64)[::-1] * 5, np.arange(64) * 3)
    add(rs.randint(0, 4, 64) << 5, rs.randint(0, 3, 64))                       # many ties
    for cnt in range(65):                                                      # 0xFFFF padding behind cnt real keys
        a = np.full(64, 0xFFFF)
        b = np.full(64, 0xFFFF)
        a[:cnt] = rs.randint(0, 8192, cnt)
        b[:min(cnt + 1, 64)] = rs.randint(0, 8192, min(cnt + 1, 64))
        rs.shuffle(a)
        add(a, b)
    for cnt in range(33):                                                      # the same inside every segment's first lanes
        a = np.full(64, 0xFFFF)
        b = np.full(64, 0xFFFF)
        for wd in (8, 16, 32):
            if cnt <= wd:
                for s0 in range(0, 64, wd):
                    a[s0:s0 + cnt] = rs.randint(0, 8192, cnt)
                    b[s0:s0 + cnt] = rs.randint(0, 8192, cnt)
        add(a, b)
    return np.stack(lo), np.stack(hi)


def test_packed_sort_networks():
    """wave_ops.h bitonic64_pk16 and forest.hip bitonic_seg_pk16<8 / 16 / 32>: each 16-bit half
    of the result is numpy's sort of that half of the input, over the wave and over each segment."""
    lib = native.hip_lib()
    fn = lib.dml_test_pk16_sorts
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lo, hi = _sort_inputs()
    nb = len(lo)
    x = (lo | (hi << 16)).astype(np.uint32)
    xd = torch.from_numpy(x.view(np.int32)).cuda()
    out = torch.empty((nb, 4, 64), dtype=torch.int32, device="cuda")
    assert fn(xd.data_ptr(), out.data_ptr(), nb, native.stream_handle()) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    for bi in range(nb):
        for half, v in ((0, lo[bi]), (1, hi[bi])):
            got = (o[bi] >> (16 * half)) & 0xFFFF
            assert np.array_equal(got[0], np.sort(v)), (bi, half)
            for row, wd in ((1, 8), (2, 16), (3, 32)):
                want = np.sort(v.reshape(64 // wd, wd), axis=1).reshape(64)
                assert np.array_equal(got[row], want), (bi, half, wd)

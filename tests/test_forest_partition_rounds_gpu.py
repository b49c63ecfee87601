"""Round structure of the block tier's two-pass partition (forest.hip k_nodes<NT > 64> pass 1,
DML_PART_STRAIGHT), its chunked fallback, the decision's refused and leaf-children outcomes, and
the subtree tier with and without its LDS row cache (subtree_dfs).  Every spec is built on the
host and on the GPU; trees must agree node for node and predictions exactly.

Pass 1 of the partition walks a node in rounds of U = 4 positions per thread: 512 rows per round
in the binary kernel (128 threads), 1024 in the three-class and regression kernels (256 threads).
The row ids of the first two rounds are kept in registers for pass 2, so the third round (row 1025
resp. 2049) is the first that is not kept.  A round's loads are clamped to the node's last row, so
the sizes that matter are a full round, one row less and one row more, at each of these borders.

Common setup: the root is itself a block-tier node (no bootstrap: every row is active; wave_max
255), 4 trees, and one constant column: a node that meets it among its first max_features
visiting positions needs a second feature group, and a split found there is past the stash, so
the partition gathers the split bins from the table (max_features 20 always has a second group,
the stash holds 16 positions; max_features 10 splits in the stash unless it met the constant
column)."""
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

NMAX = 22003
COLCONST = 3
NTREES = 4
SQUARED_ERROR = 2
DS = (24, 100)


@functools.lru_cache(maxsize=None)
def _table(D):
    """Bins drawn directly (no quantiser), one constant column.  Labels and targets depend on a few
    columns plus noise, so no node is pure before it is small; `noise` labels depend on nothing.
    An N-row case uses the first N rows."""
    rs = np.random.RandomState(977 + D)
    Xb = rs.randint(0, 256, size=(NMAX, D)).astype(np.uint8)
    Xb[:, COLCONST] = 77
    s = (Xb[:, 2] > 128).astype(np.int32) + (Xb[:, 7] > 60) + (Xb[:, 15] > 200)
    y2 = ((s & 1) ^ (rs.rand(NMAX) < 0.15)).astype(np.int32)
    y3 = np.where(rs.rand(NMAX) < 0.15, rs.randint(0, 3, size=NMAX), s % 3).astype(np.int32)
    yr = (Xb[:, 2] * 0.05 + (Xb[:, 7] > 60) * 3.0 + Xb[:, 15] * Xb[:, 21] * 1e-4 + rs.randn(NMAX)).astype(np.float32)
    noise = rs.randint(0, 2, size=NMAX).astype(np.int32)
    return np.ascontiguousarray(Xb), {"bin": y2, "mc": y3, "reg": yr, "noise": noise}


def _specs(criterion, k, msl=None, mid=0.0):
    specs = forest_ops.make_specs(NTREES)
    for t in range(NTREES):
        s = specs[t]
        s["seed"] = 7331 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = (1 + 2 * (t % 2)) if msl is None else msl
        s["max_features"] = k
        s["bootstrap"] = 0
        s["criterion"] = criterion
        s["min_impurity_decrease"] = mid
        s["pois_cdf"] = native.poisson_cdf_table(1.0)
    return specs


def _walk(nodes, vals, T):
    """Per tree, the preorder (split word, rounded values) sequence; and the set of reached nodes."""
    out, seen = [], set()
    for t in range(T):
        seq, stack = [], [t]
        while stack:
            i = stack.pop()
            seen.add(i)
            s, l = int(nodes[i, 0]), int(nodes[i, 1])
            seq.append((s, tuple(np.round(vals[i], 6))))
            if s >= 0:
                stack.append(l + 1)
                stack.append(l)
        out.append(seq)
    return out, seen


def _target(task, D, N):
    y = _table(D)[1][task]
    if task == "reg":
        return None, np.ascontiguousarray(y[:N]), 1, True
    return np.ascontiguousarray(y[:N]), None, (3 if task == "mc" else 2), False


@functools.lru_cache(maxsize=None)
def _host(task, criterion, D, N, k, msl, mid):
    """The host builder's trees and predictions of one spec, computed once."""
    Xb_cpu = np.ascontiguousarray(_table(D)[0][:N])
    ycls, yreg, C, is_reg = _target(task, D, N)
    roles = np.ones((1, N), dtype=np.uint8)
    c = forest_ops.build_cpu(Xb_cpu, ycls, yreg, roles, _specs(criterion, k, msl, mid), C, is_reg)
    rows = np.arange(N, dtype=np.int32)
    pc = forest_ops.predict(c, Xb_cpu, np.array([0, NTREES]), np.array([0, N]), rows)
    return _walk(c.nodes, c.vals, NTREES)[0], c.stats["nodes"], pc


def _compare(task, criterion, D, N, k, msl=None, mid=0.0, tiers=None, block_root=True):
    """Builds on the GPU, compares with the host, and returns the GPU build."""
    ycls, yreg, C, is_reg = _target(task, D, N)
    cc, cn, pc = _host(task, criterion, D, N, k, msl, mid)
    dev = torch.device("cuda:0")
    # 24 columns: pitch 24 (below 112: byte gathers); 100 columns on 128 bytes, the bench's layout
    pitch = 128 if D == 100 else D
    buf = torch.zeros((N, pitch), dtype=torch.uint8, device=dev)
    buf[:, :D] = torch.from_numpy(_table(D)[0][:N]).to(dev)
    Xb = buf[:, :D]
    roles = torch.ones((1, N), dtype=torch.uint8, device=dev)
    g = forest_ops.build_gpu(Xb, None if ycls is None else torch.from_numpy(ycls).to(dev),
                             None if yreg is None else torch.from_numpy(yreg).to(dev), roles,
                             _specs(criterion, k, msl, mid), C, is_reg,
                             forest_ops.ForestTiers(**dict(dict(wave_max=255), **(tiers or {}))))
    if block_root:
        assert g.stats["tier_nodes"][2] > 0          # block-tier nodes were handled
        assert g.stats["tier_nodes"][3] == 0         # and no large-tier node
    gn = g.nodes.cpu().numpy()
    gc, seen = _walk(gn, g.vals.cpu().numpy(), NTREES)
    # a reserved child pair that no split took stays two unreferenced LEAVES
    for i in range(gn.shape[0]):
        if i not in seen:
            assert int(gn[i, 0]) == -1 and int(gn[i, 1]) == -1, i
    assert sum(map(len, gc)) == sum(map(len, cc)) == cn
    assert gc == cc
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    pg = forest_ops.predict(g, Xb, np.array([0, NTREES]), np.array([0, N]), rows).cpu().numpy()
    assert np.array_equal(pg, pc)
    return g, cc


# ---- round boundaries ------------------------------------------------------------------------

@pytest.mark.parametrize("k", (10, 20))
@pytest.mark.parametrize("N", (511, 512, 513, 1024, 1025, 1536, 1537, 2049))
@pytest.mark.parametrize("D", DS)
def test_partition_rounds_binary_match_host(D, N, k):
    """128 threads, rounds of 512 rows: one round less a row, exactly, plus a row; two kept rounds;
    1025: the first round that is not kept; three and four rounds, and a fifth of one row."""
    _compare("bin", forest_ops.GINI, D, N, k)


@pytest.mark.parametrize("k", (10, 20))
@pytest.mark.parametrize("N", (1024, 1025, 2048, 2049, 3073))
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("task,criterion", (("mc", forest_ops.GINI), ("reg", SQUARED_ERROR)))
def test_partition_rounds_256_threads_match_host(task, criterion, D, N, k):
    """256 threads, rounds of 1024 rows: 2049 is the first round that is not kept."""
    _compare(task, criterion, D, N, k)


# ---- chunked fallback ------------------------------------------------------------------------

@pytest.mark.parametrize("task,N", (("bin", 20011), ("mc", 20011), ("mc", NMAX)))
def test_partition_chunked_fallback_matches_host(task, N):
    """max_features 1: the block kernel's histogram slab is ONE feature's histogram, and the
    two-pass partition needs 12 B of it per 64 rows.  Binary: 256 packed u64 words = 2048 B, so
    nodes above 64 * floor(2048 / 12) = 10 880 rows take the chunked partition: the 20 011-row
    root (ceil(20011 / 64) * 12 = 3756 B) and its larger children.  Three classes: 4 planes of
    256 u32 = 4096 B holds the flags of 21 824 rows; the 20 011-row root still fits (two-pass,
    gpt = 2 groups per thread in the offset scan), the 22 003-row root (344 * 12 = 4128 B) does
    not.  Smaller nodes of the same trees take the two-pass path, so both meet in every tree."""
    _compare(task, forest_ops.GINI, 24, N, 1)


# ---- subtree tier, with and without the LDS row cache -------------------------------------------

@pytest.mark.parametrize("cache_d", (0, 256))
@pytest.mark.parametrize("N", (9, 33, 64))
@pytest.mark.parametrize("task,criterion", (("bin", forest_ops.GINI), ("bin", forest_ops.ENTROPY),
                                            ("reg", SQUARED_ERROR)))
def test_subtree_cache_choice_matches_host(task, criterion, N, cache_d):
    """The root is a subtree-tier node: 9 rows (segments of 16 lanes when cached), 33 (above the
    segmented evaluation and the small-subtree tier) and 64 (a full wave).  sub_cache_max_d 0:
    every bin is read from the table; 256: from the LDS row cache (the control)."""
    g, _ = _compare(task, criterion, 24, N, 10, msl=1, tiers=dict(sub_cache_max_d=cache_d), block_root=False)
    assert g.stats["tier_nodes"][2] == 0 and g.stats["tier_nodes"][3] == 0


# ---- decision outcomes that write no children --------------------------------------------------

def test_refused_root_split_leaves_two_unreferenced_leaves():
    """Labels that depend on no column and min_impurity_decrease 0.05: the root (2049 rows, a
    block-tier node; the best of 10 x 255 candidate splits of pure noise gains about 10 / (2 N)
    = 0.0025 in Gini) finds a split and refuses it.  Every tree is its root.  The build returns the
    whole node pool, so each root's reserved pair is in it: 3 nodes per tree, the pair two leaves
    that nothing references (checked in _compare for every node outside the trees)."""
    g, cc = _compare("noise", forest_ops.GINI, 24, 2049, 10, mid=0.05)
    assert all(len(seq) == 1 for seq in cc)
    assert g.nodes.shape[0] == 3 * NTREES


def test_refused_splits_below_the_root():
    """Labels with signal and min_impurity_decrease 0.002: trees whose root meets a signal column
    accept the top splits, and their block-tier nodes further down, where only the 15 % label
    noise is left, refuse theirs (a few nodes per tree where thousands would grow)."""
    _, cc = _compare("bin", forest_ops.GINI, 24, 6001, 10, mid=0.002)
    assert max(len(seq) for seq in cc) >= 3 and all(len(seq) < 200 for seq in cc)


def test_both_children_leaves_by_min_samples_leaf():
    """513 rows, min_samples_leaf 200: the root splits (no child below 200 rows) and neither
    child can (fewer than 400 rows): both stage records are closed, each tree has 3 nodes."""
    _, cc = _compare("bin", forest_ops.GINI, 24, 513, 10, msl=200)
    assert all(len(seq) == 3 for seq in cc)

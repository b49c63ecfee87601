"""The block tier's bin stash as dword planes (forest.hip k_nodes<NT > 64>, DML_BLOCK_STASH_PLANES;
forest_common.h stash_plane_base): the histogram pass of a block-tier node stores the bins of its
first feature group as ceil(g / 4) planes of one word per row position inside the node's own
scratch range, and the partition reads the split position's plane.  Every spec is built on the
host and on the GPU; trees must agree node for node and predictions exactly.

Shapes are the smallest at which this code can go wrong.  The root is itself a block-tier node
(no bootstrap: every row is active; wave_max 255 for every task): 256 rows (the smallest block
node), 257, 1153 (past the 1024 rows whose ids the binary kernel's partition keeps from pass 1,
ragged in its last 128-row chunk), 6001, and 20 011 (above 128 x 128 rows: the group-offset scan
of the two-pass partition walks more than two groups per thread -- docs/ROUND3.md records a bug
in exactly that place).  Two tables: 24 columns (row pitch 24: byte gathers) and 100 columns on
a 128-byte pitch (whole-row windows for first groups of >= 8 features).  One column is constant,
so a node that meets it among its first max_features visiting positions needs a second group,
and a split found there is past the stash: the partition gathers it from the table."""
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

NMAX = 20011
COLCONST = 3
NTREES = 4
SQUARED_ERROR = 2
TIERS = dict(wave_max=255)        # block_max stays at its default: no large-tier node below 65 537 rows
DS = (24, 100)
ROWS = (256, 257, 1153, 6001, NMAX)
# 3: one partly filled plane; 8: two full planes (smallest row-window group); 10: third plane
# partly filled; 16: four planes, the node's range filled exactly; 20: two groups
KS = (3, 8, 10, 16, 20)


@functools.lru_cache(maxsize=None)
def _table(D):
    """Bins drawn directly (no quantiser), one constant column; labels and targets that depend on
    a few columns plus noise, so no node is pure before it is small.  An N-row case uses the
    first N rows."""
    rs = np.random.RandomState(41 + D)
    Xb = rs.randint(0, 256, size=(NMAX, D)).astype(np.uint8)
    Xb[:, COLCONST] = 77
    s = (Xb[:, 2] > 128).astype(np.int32) + (Xb[:, 7] > 60) + (Xb[:, 15] > 200)
    y2 = ((s & 1) ^ (rs.rand(NMAX) < 0.15)).astype(np.int32)
    y3 = np.where(rs.rand(NMAX) < 0.15, rs.randint(0, 3, size=NMAX), s % 3).astype(np.int32)
    yr = (Xb[:, 2] * 0.05 + (Xb[:, 7] > 60) * 3.0 + Xb[:, 15] * Xb[:, 21] * 1e-4 + rs.randn(NMAX)).astype(np.float32)
    return np.ascontiguousarray(Xb), y2, y3, yr


def _specs(criterion, k, bootstrap):
    specs = forest_ops.make_specs(NTREES)
    for t in range(NTREES):
        s = specs[t]
        s["seed"] = 4409 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = 1 + 2 * (t % 2)
        s["max_features"] = k
        s["bootstrap"] = bootstrap
        s["criterion"] = criterion
        s["pois_cdf"] = native.poisson_cdf_table(1.0)
    return specs


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


def _target(task, D, N):
    _, y2, y3, yr = _table(D)
    if task == "reg":
        return None, np.ascontiguousarray(yr[:N]), 1, True
    y = y2 if task == "bin" else y3
    return np.ascontiguousarray(y[:N]), None, (2 if task == "bin" else 3), False


@functools.lru_cache(maxsize=None)
def _host(task, criterion, D, N, k, bootstrap):
    """The host builder's trees and predictions of one spec, computed once."""
    Xb_cpu = np.ascontiguousarray(_table(D)[0][:N])
    ycls, yreg, C, is_reg = _target(task, D, N)
    roles = np.ones((1, N), dtype=np.uint8)
    c = forest_ops.build_cpu(Xb_cpu, ycls, yreg, roles, _specs(criterion, k, bootstrap), C, is_reg)
    rows = np.arange(N, dtype=np.int32)
    pc = forest_ops.predict(c, Xb_cpu, np.array([0, NTREES]), np.array([0, N]), rows)
    return _canon(c.nodes, c.vals, NTREES), c.stats["nodes"], pc


def _compare(task, criterion, D, N, k, bootstrap):
    assert native.hip_lib().dml_forest_block_stash_planes() == 1
    ycls, yreg, C, is_reg = _target(task, D, N)
    cc, cn, pc = _host(task, criterion, D, N, k, bootstrap)
    dev = torch.device("cuda:0")
    # 24 columns: pitch 24 (below 112: byte gathers); 100 columns on 128 bytes, the bench's layout
    pitch = 128 if D == 100 else D
    buf = torch.zeros((N, pitch), dtype=torch.uint8, device=dev)
    buf[:, :D] = torch.from_numpy(_table(D)[0][:N]).to(dev)
    Xb = buf[:, :D]
    roles = torch.ones((1, N), dtype=torch.uint8, device=dev)
    g = forest_ops.build_gpu(Xb, None if ycls is None else torch.from_numpy(ycls).to(dev),
                             None if yreg is None else torch.from_numpy(yreg).to(dev), roles,
                             _specs(criterion, k, bootstrap), C, is_reg, forest_ops.ForestTiers(**TIERS))
    assert g.stats["tier_nodes"][2] > 0          # block-tier nodes were split
    assert g.stats["tier_nodes"][3] == 0         # and no large-tier node
    gc = _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), NTREES)
    assert sum(map(len, gc)) == sum(map(len, cc)) == cn
    assert gc == cc
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    pg = forest_ops.predict(g, Xb, np.array([0, NTREES]), np.array([0, N]), rows).cpu().numpy()
    assert np.array_equal(pg, pc)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("D", DS)
def test_block_planes_binary_gini_matches_host(D, N, k):
    _compare("bin", forest_ops.GINI, D, N, k, 0)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("D", DS)
def test_block_planes_binary_bootstrap_matches_host(D, k):
    """Bootstrap on at 6001 rows: the root holds the rows of non-zero weight only."""
    _compare("bin", forest_ops.GINI, D, 6001, k, 1)


@pytest.mark.parametrize("k", (10, 20))
@pytest.mark.parametrize("N", (257, NMAX))
@pytest.mark.parametrize("D", DS)
def test_block_planes_binary_entropy_matches_host(D, N, k):
    _compare("bin", forest_ops.ENTROPY, D, N, k, 0)


# three classes and regression run the 256-thread block kernels
@pytest.mark.parametrize("k", (3, 10, 16, 20))
@pytest.mark.parametrize("N", (256, 1153, NMAX))
@pytest.mark.parametrize("D", DS)
def test_block_planes_three_classes_match_host(D, N, k):
    _compare("mc", forest_ops.GINI, D, N, k, 0)


@pytest.mark.parametrize("k", (3, 10, 16, 20))
@pytest.mark.parametrize("N", (256, 1153, NMAX))
@pytest.mark.parametrize("D", DS)
def test_block_planes_regression_matches_host(D, N, k):
    _compare("reg", SQUARED_ERROR, D, N, k, 0)

"""The large tier without per-row bin slots (forest.hip k_hist_large / k_partition_large,
DML_LARGE_STASH 0): a build that has the feature-major table stores no 16-byte `bscr` slot in
its feature-subset rounds and its partition reads the split feature's bytes from the table.
Every spec is built three times -- host, GPU without the table (slots kept) and GPU with it
(no slots) -- and the three must agree node for node and prediction for prediction.

Tiers are shrunk so that the top four levels of a 6001-row table are large-tier nodes cut into
256-row chunks with a ragged last one (6001 = 23 x 256 + 113)."""
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

N, D = 6001, 24
COLCONST = 3          # among the first visiting positions of some nodes: extra positions, a later round
TIERS = dict(sub_max=64, wave_max=255, block_max=512, chunk=256, chunk_reg=256)
NTREES = 6
SQUARED_ERROR = 2


@functools.lru_cache(maxsize=None)
def _table():
    """Bins drawn directly (no quantiser), one constant column; labels and targets that depend
    on a few columns plus noise, so no node is pure before it is small."""
    rs = np.random.RandomState(23)
    Xb = rs.randint(0, 256, size=(N, D)).astype(np.uint8)
    Xb[:, COLCONST] = 77
    s = (Xb[:, 2] > 128).astype(np.int32) + (Xb[:, 7] > 60) + (Xb[:, 15] > 200)
    y2 = ((s & 1) ^ (rs.rand(N) < 0.15)).astype(np.int32)
    y3 = np.where(rs.rand(N) < 0.15, rs.randint(0, 3, size=N), s % 3).astype(np.int32)
    yr = (Xb[:, 2] * 0.05 + (Xb[:, 7] > 60) * 3.0 + Xb[:, 15] * Xb[:, 21] * 1e-4 + rs.randn(N)).astype(np.float32)
    return np.ascontiguousarray(Xb), y2, y3, yr


def _specs(criterion, k, bootstrap):
    specs = forest_ops.make_specs(NTREES)
    for t in range(NTREES):
        s = specs[t]
        s["seed"] = 977 + t
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


def _target(task):
    Xb_cpu, y2, y3, yr = _table()
    if task == "reg":
        return None, yr, 1, True
    return (y2 if task == "bin" else y3), None, (2 if task == "bin" else 3), False


@functools.lru_cache(maxsize=None)
def _host(task, criterion, k, bootstrap):
    """The host builder's trees and predictions of one spec: computed once, shared by both GPU legs."""
    Xb_cpu = _table()[0]
    ycls, yreg, C, is_reg = _target(task)
    specs = _specs(criterion, k, bootstrap)
    roles = np.ones((1, N), dtype=np.uint8)
    c = forest_ops.build_cpu(Xb_cpu, ycls, yreg, roles, specs, C, is_reg)
    rows = np.arange(N, dtype=np.int32)
    pc = forest_ops.predict(c, Xb_cpu, np.array([0, NTREES]), np.array([0, N]), rows)
    return _canon(c.nodes, c.vals, NTREES), c.stats["nodes"], pc


def _compare(task, criterion, k, bootstrap, with_table):
    Xb_cpu = _table()[0]
    ycls, yreg, C, is_reg = _target(task)
    cc, cn, pc = _host(task, criterion, k, bootstrap)
    dev = torch.device("cuda:0")
    if with_table:   # the library under test drops the slots when it has the table
        assert native.hip_lib().dml_forest_large_stash() == 0
    Xb = torch.from_numpy(Xb_cpu).to(dev)
    XbT = Xb.t().contiguous() if with_table else None
    roles = torch.ones((1, N), dtype=torch.uint8, device=dev)
    g = forest_ops.build_gpu(Xb, None if ycls is None else torch.from_numpy(ycls).to(dev),
                             None if yreg is None else torch.from_numpy(yreg).to(dev), roles,
                             _specs(criterion, k, bootstrap), C, is_reg, forest_ops.ForestTiers(**TIERS), XbT=XbT)
    assert g.stats["tier_nodes"][3] > 0          # large-tier nodes were split
    gc = _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), NTREES)
    assert sum(map(len, gc)) == sum(map(len, cc)) == cn
    assert gc == cc
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    pg = forest_ops.predict(g, Xb, np.array([0, NTREES]), np.array([0, N]), rows).cpu().numpy()
    assert np.array_equal(pg, pc)


# 5, 10: one round of the visiting order unless the constant column costs a position (then the
# best split can come from a second round, past the slots); 20: two rounds (kg_large 16);
# 24: every feature -- whole-histogram levels, which keep their slots with the table too
@pytest.mark.parametrize("with_table", [False, True], ids=["slots", "table"])
@pytest.mark.parametrize("k", [5, 10, 20, 24])
@pytest.mark.parametrize("bootstrap", [1, 0])
@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
def test_large_tier_binary_matches_host(criterion, bootstrap, k, with_table):
    _compare("bin", criterion, k, bootstrap, with_table)


@pytest.mark.parametrize("with_table", [False, True], ids=["slots", "table"])
def test_large_tier_three_classes_match_host(with_table):
    _compare("mc", forest_ops.GINI, 10, 1, with_table)


@pytest.mark.parametrize("with_table", [False, True], ids=["slots", "table"])
@pytest.mark.parametrize("bootstrap", [1, 0])        # 0: the unit-weight (compact / packed) histogram slices
def test_large_tier_regression_matches_host(bootstrap, with_table):
    _compare("reg", SQUARED_ERROR, 10, bootstrap, with_table)

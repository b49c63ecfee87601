"""Histogram pass of short block-tier nodes (forest.hip k_nodes<NT > 64>, DML_HIST_SHORT): the
chunk pipeline of the row-window path (one row per thread per chunk of NT rows) loads the row lines
of a node's ceil(cnt / NT) chunks and of no chunk behind them; inside the last, partial chunk a
lane past the node's last row reads row 0's line and adds nothing.  Every spec is built on the host
and on the GPU; trees must agree node for node and predictions exactly.

The roots are themselves block-tier nodes (no bootstrap: every row is active; wave_max 256) of a
full chunk, one row less and one row more, at the borders between 2 .. 6 chunks: NT = 128 in the
binary kernels, 256 in the three-class and regression kernels.  The children of these roots walk
the sizes below them.  d = 100 on the 128-B pitch with max_features 10 is the row-window path (first
group of >= 8 features); d = 20 with max_features 4 gathers bytes.  At most 8 trees per case."""
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

NMAX = 1025
NTREES = 8
SQUARED_ERROR = 2
TIERS = dict(wave_max=256)


@functools.lru_cache(maxsize=None)
def _table(D):
    """Bins drawn directly (no quantiser).  Labels and targets depend on a few columns plus noise,
    so no node is pure before it is small.  An N-row case uses the first N rows."""
    rs = np.random.RandomState(1409 + D)
    Xb = rs.randint(0, 256, size=(NMAX, D)).astype(np.uint8)
    s = (Xb[:, 2] > 128).astype(np.int32) + (Xb[:, 7] > 60) + (Xb[:, 15] > 200)
    y2 = ((s & 1) ^ (rs.rand(NMAX) < 0.15)).astype(np.int32)
    y3 = np.where(rs.rand(NMAX) < 0.15, rs.randint(0, 3, size=NMAX), s % 3).astype(np.int32)
    yr = (Xb[:, 2] * 0.05 + (Xb[:, 7] > 60) * 3.0 + Xb[:, 15] * Xb[:, 11] * 1e-4 + rs.randn(NMAX)).astype(np.float32)
    return np.ascontiguousarray(Xb), {"bin": y2, "mc": y3, "reg": yr}


def _specs(criterion, k, cw_mode):
    specs = forest_ops.make_specs(NTREES)
    for t in range(NTREES):
        s = specs[t]
        s["seed"] = 4177 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = 1 + 2 * (t % 2)
        s["max_features"] = k
        s["bootstrap"] = 0
        s["criterion"] = criterion
        s["cw_mode"] = cw_mode
        s["pois_cdf"] = native.poisson_cdf_table(1.0)
    return specs


def _class_weights(cw_mode):
    return None if cw_mode == 0 else np.tile(np.array([1.0, 3.5]), (NTREES, 1))


def _walk(nodes, vals, T):
    """Per tree, the preorder (split word, rounded values) sequence."""
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
    y = _table(D)[1][task]
    if task == "reg":
        return None, np.ascontiguousarray(y[:N]), 1, True
    return np.ascontiguousarray(y[:N]), None, (3 if task == "mc" else 2), False


@functools.lru_cache(maxsize=None)
def _host(task, criterion, D, N, k, cw_mode):
    """The host builder's trees and predictions of one spec, computed once."""
    Xb_cpu = np.ascontiguousarray(_table(D)[0][:N])
    ycls, yreg, C, is_reg = _target(task, D, N)
    roles = np.ones((1, N), dtype=np.uint8)
    c = forest_ops.build_cpu(Xb_cpu, ycls, yreg, roles, _specs(criterion, k, cw_mode), C, is_reg,
                             cw=_class_weights(cw_mode))
    rows = np.arange(N, dtype=np.int32)
    pc = forest_ops.predict(c, Xb_cpu, np.array([0, NTREES]), np.array([0, N]), rows)
    return _walk(c.nodes, c.vals, NTREES), c.stats["nodes"], pc


def _compare(task, criterion, D, N, k, cw_mode=0):
    ycls, yreg, C, is_reg = _target(task, D, N)
    cc, cn, pc = _host(task, criterion, D, N, k, cw_mode)
    dev = torch.device("cuda:0")
    # 100 columns on 128 bytes, the bench's layout (row windows); 20 columns: pitch 20, byte gathers
    pitch = 128 if D == 100 else D
    buf = torch.zeros((N, pitch), dtype=torch.uint8, device=dev)
    buf[:, :D] = torch.from_numpy(_table(D)[0][:N]).to(dev)
    Xb = buf[:, :D]
    roles = torch.ones((1, N), dtype=torch.uint8, device=dev)
    g = forest_ops.build_gpu(Xb, None if ycls is None else torch.from_numpy(ycls).to(dev),
                             None if yreg is None else torch.from_numpy(yreg).to(dev), roles,
                             _specs(criterion, k, cw_mode), C, is_reg, forest_ops.ForestTiers(**TIERS),
                             cw=_class_weights(cw_mode))
    assert g.stats["tier_nodes"][2] >= NTREES      # every root was a block-tier node
    assert g.stats["tier_nodes"][3] == 0           # and no large-tier node
    gc = _walk(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), NTREES)
    assert sum(map(len, gc)) == sum(map(len, cc)) == cn
    assert gc == cc
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    pg = forest_ops.predict(g, Xb, np.array([0, NTREES]), np.array([0, N]), rows).cpu().numpy()
    assert np.array_equal(pg, pc)


@pytest.mark.parametrize("N", (257, 383, 384, 385, 511, 512, 513, 640, 641))
def test_row_window_path_binary_matches_host(N):
    """NT = 128: 3 chunks (257 .. 384), 4 (385 .. 512), 5 (513 .. 640), 6 (641)."""
    _compare("bin", forest_ops.GINI, 100, N, 10)


@pytest.mark.parametrize("N", (257, 385, 513, 641))
def test_byte_gather_path_binary_matches_host(N):
    """d = 20, max_features 4: the first group is below 8 features and gathers bytes."""
    _compare("bin", forest_ops.GINI, 20, N, 4)


@pytest.mark.parametrize("N", (513, 768, 769, 1025))
@pytest.mark.parametrize("task,criterion", (("mc", forest_ops.GINI), ("reg", SQUARED_ERROR)))
def test_256_thread_kernels_match_host(task, criterion, N):
    """NT = 256: 3 chunks (513 .. 768), 4 (769), 5 (1025)."""
    _compare(task, criterion, 100, N, 10)


def test_class_weight_matches_host():
    """class_weight: the generic-criterion (FC = -1) binary block kernel."""
    _compare("bin", forest_ops.GINI, 100, 385, 10, cw_mode=1)


def test_entropy_matches_host():
    """criterion="entropy": the generic-criterion binary block kernel."""
    _compare("bin", forest_ops.ENTROPY, 100, 513, 10)

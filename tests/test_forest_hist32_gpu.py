"""The binary wave tier's 32-bit packed histogram word (forest.hip k_nodes<64, 1, FC, true>,
forest_common.h pack_bin32) against the host builder: node-for-node equal trees and
bit-for-bit equal predictions, at the row counts where the narrow word and its tier
boundary can go wrong (255 rows: the largest node it holds; 256: the first block-tier node;
65: the smallest wave-tier node)."""
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

N, D = 4000, 24
COL255, COL256, COL65, COLCONST = 3, 11, 17, 20
TIERS = dict(sub_max=64, wave_max=255, block_max=1024, chunk=512)
NTREES = 8


@functools.lru_cache(maxsize=None)
def _table():
    """Bins (drawn directly, no quantiser) and labels.  The rows fall into three regions, cut
    into runs of 255, 256 and 65 rows by one column each (255 outside its region); the label is
    the parity of a row's run number with 12 % of the rows flipped.  A tree that sees the run
    columns splits on them until single runs are left, and a run is never pure, so it is split
    again: split nodes of exactly 255, 256 and 65 rows.  One column is constant (it takes a
    visiting position but does not count towards max_features: the extra-position path)."""
    rs = np.random.RandomState(11)
    idx = np.arange(N)
    Xb = rs.randint(0, 256, size=(N, D)).astype(np.uint8)
    a, b = 6 * 255, 6 * 255 + 6 * 256
    run = np.where(idx < a, idx // 255, np.where(idx < b, (idx - a) // 256, (idx - b) // 65))
    Xb[:, COL255] = np.where(idx < a, run, 255)
    Xb[:, COL256] = np.where((idx >= a) & (idx < b), run, 255)
    Xb[:, COL65] = np.where(idx >= b, run, 255)
    Xb[:, COLCONST] = 77
    y = (run & 1) ^ (rs.rand(N) < 0.12)
    return np.ascontiguousarray(Xb), y.astype(np.int32)


def _shifted_poisson_table():
    """1 + Poisson(1) weights (1..12): a bootstrap that keeps every row, so a node's row count
    is the number of rows routed to it while the weights still differ from row to row."""
    t = native.poisson_cdf_table(1.0).astype(np.uint32)
    return np.concatenate([np.zeros(1, np.uint32), t[:-1]])


def _specs(ntrees, criterion, msl, k, bootstrap, keep_rows):
    specs = forest_ops.make_specs(ntrees)
    for t in range(ntrees):
        s = specs[t]
        s["seed"] = 4242 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = msl
        s["max_features"] = k
        s["bootstrap"] = bootstrap
        s["criterion"] = criterion
        # even trees: the 1 + Poisson table (row counts known); odd trees: plain Poisson(1)
        s["pois_cdf"] = _shifted_poisson_table() if (keep_rows and t % 2 == 0) else native.poisson_cdf_table(1.0)
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


def _split_node_rows(nodes, Xb, root):
    """Row counts of the internal (split) nodes of one tree that keeps every row."""
    counts, stack = [], [(root, np.arange(len(Xb)))]
    while stack:
        i, rows = stack.pop()
        s, l = int(nodes[i, 0]), int(nodes[i, 1])
        if s < 0:
            continue
        counts.append(len(rows))
        left = Xb[rows, s // 256] <= (s % 256)
        stack.append((l, rows[left]))
        stack.append((l + 1, rows[~left]))
    return counts


def _compare(specs, cw=None):
    Xb_cpu, ycls = _table()
    dev = torch.device("cuda:0")
    assert native.hip_lib().dml_forest_wave_hist32() == 1      # the library under test has the narrow kernel
    Xb = torch.from_numpy(Xb_cpu).to(dev)
    roles = np.ones((1, N), dtype=np.uint8)                     # every row trains
    T = len(specs)
    kw = {} if cw is None else {"cw": cw.copy()}
    g = forest_ops.build_gpu(Xb, torch.from_numpy(ycls).to(dev), None, torch.from_numpy(roles).to(dev), specs, 2, False,
                             forest_ops.ForestTiers(**TIERS), **kw)
    c = forest_ops.build_cpu(Xb_cpu, ycls, None, roles, specs, 2, False, **kw)
    assert g.stats["tier_nodes"][1] > 0 and g.stats["tier_nodes"][2] > 0
    gc = _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), T)
    cc = _canon(c.nodes, c.vals, T)
    assert sum(map(len, gc)) == sum(map(len, cc)) == c.stats["nodes"]
    assert gc == cc
    rows = np.arange(N, dtype=np.int32)
    roff, toff = np.array([0, N]), np.array([0, T])
    pg = forest_ops.predict(g, Xb, toff, roff, torch.from_numpy(rows).to(dev)).cpu().numpy()
    pc = forest_ops.predict(c, Xb_cpu, toff, roff, rows)
    assert np.array_equal(pg, pc)
    return c


@pytest.mark.parametrize("k", [5, 10, 24])          # 24: more feature groups than kg_wave holds
@pytest.mark.parametrize("msl", [1, 8])
@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
def test_narrow_wave_tier_matches_host(criterion, msl, k):
    specs = _specs(NTREES, criterion, msl, k, bootstrap=1, keep_rows=True)
    c = _compare(specs)
    # the host builder's trees (those that keep every row) hold split nodes of exactly 255, 256
    # and 65 rows: the narrow word's largest node, the first block-tier one, the smallest wave-tier one
    Xb_cpu, _ = _table()
    counts = []
    for t in range(0, NTREES, 2):
        counts += _split_node_rows(c.nodes, Xb_cpu, t)
    assert {255, 256, 65} <= set(counts), sorted(set(counts) & set(range(60, 260)))


@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
def test_narrow_wave_tier_unit_weights(criterion):
    _compare(_specs(NTREES, criterion, 1, 10, bootstrap=0, keep_rows=False))


@pytest.mark.parametrize("msl", [1, 8])
def test_narrow_wave_tier_class_weights(msl):
    """class_weight (dict rows and balanced_subsample): the narrow word holds the integer sums,
    the weights multiply them at evaluation."""
    specs = _specs(NTREES, forest_ops.GINI, msl, 10, bootstrap=1, keep_rows=True)
    cw = np.ones((NTREES, 2))
    for t in range(NTREES):
        specs[t]["cw_mode"] = (0, 1, 2)[t % 3]
        if t % 3 == 1:
            cw[t] = (1.0, 3.5)
    _compare(specs, cw=cw)

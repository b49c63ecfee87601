"""Trees grown with the segmented binary Gini split search (forest.hip eval_gini_seg: the wave
and block tiers score two or four features of a group per wave pass) against the host builder:
node-for-node equal trees and bit-for-bit equal predictions, at every max_features that gives a
wave its share of a feature group as fours, pairs and a single in another mix, with Gini
(specialised kernels), Gini with class weights (generic kernels) and entropy (the one-feature
loop, unchanged)."""
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

N, D = 4000, 24
COLCONST = 20
TIERS = dict(sub_max=64, wave_max=255, block_max=1024, chunk=512)
NTREES = 8


@functools.lru_cache(maxsize=None)
def _table():
    """Bins drawn directly and a noisy label of three columns (so nodes of every size down to
    the subtree tier stay impure).  One column is constant: it takes a visiting position in a
    feature group but does not count towards max_features."""
    rs = np.random.RandomState(23)
    Xb = rs.randint(0, 256, size=(N, D)).astype(np.uint8)
    Xb[:, 7] = rs.randint(0, 9, size=N) * 30          # few distinct bins: equal gains are common
    Xb[:, COLCONST] = 77
    y = ((Xb[:, 0] > 128) ^ (Xb[:, 5] > 60) ^ (Xb[:, 7] > 100)) ^ (rs.rand(N) < 0.15)
    return np.ascontiguousarray(Xb), y.astype(np.int32)


def _specs(criterion, msl, k):
    specs = forest_ops.make_specs(NTREES)
    for t in range(NTREES):
        s = specs[t]
        s["seed"] = 977 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = msl
        s["max_features"] = k
        s["bootstrap"] = 1
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


def _compare(specs, cw=None):
    Xb_cpu, ycls = _table()
    dev = torch.device("cuda:0")
    Xb = torch.from_numpy(Xb_cpu).to(dev)
    roles = np.ones((1, N), dtype=np.uint8)
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


def _class_weights(specs):
    cw = np.ones((NTREES, 2))
    for t in range(NTREES):
        specs[t]["cw_mode"] = (0, 1, 2)[t % 3]
        if t % 3 == 1:
            cw[t] = (0.5, 3.0)
    return cw


KS = [1, 2, 3, 5, 7, 8, 10, 11]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("msl", [1, 3])
@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
def test_trees_match_host(criterion, msl, k):
    _compare(_specs(criterion, msl, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("msl", [1, 3])
def test_trees_match_host_class_weights(msl, k):
    specs = _specs(forest_ops.GINI, msl, k)
    _compare(specs, cw=_class_weights(specs))


@pytest.mark.parametrize("k", [3, 5, 10])
@pytest.mark.parametrize("weighted", [False, True])
def test_trees_match_host_wide_wave_tier(monkeypatch, weighted, k):
    """wave_max above 255: the wave tier runs the 64-bit-word kernel."""
    monkeypatch.setenv("DML_TIER_WAVE_MAX", "400")
    specs = _specs(forest_ops.GINI, 1, k)
    _compare(specs, cw=_class_weights(specs) if weighted else None)

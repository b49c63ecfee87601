"""The subtree tier's code after the packed sort (forest.hip DML_SUB_POST: sub_post_pk2 for nodes of
33..64 rows, seg_post_pk2<8 / 16 / 32> below; docs/SUBTREE_POST.md) against the host builder, node
for node, on tables so small that the build is subtree-tier work: n in {9, 33, 64, 200} rows,
d in {3, 11, 100} features, and in every build 8 bootstrap trees for each max_features in
{1, 2, sqrt(d), d} and min_samples_leaf in {1, 4}.  Odd d and odd max_features leave the high key
half absent or uncounted on the last pass.  The tie table holds identical column pairs and a
constant column: equal scores in the two halves of one packed sort, where the earlier visiting
position must win as it does on the host.  The near-tie tables hold two scores closer than 2^-30
of their value in the two halves of one sort.  Entropy builds keep the one-half-at-a-time code and
are checked on the same tables."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.ops import forest_ops
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

TIERS = dict(sub_max=64, wave_max=255, block_max=1024, chunk=512)
PER = 8                                   # trees per (max_features, min_samples_leaf)
MSL = (1, 4)


def _max_features(d):
    return (1, 2, int(np.sqrt(d)), d)


@functools.lru_cache(maxsize=None)
def _table(n, d):
    """Bins drawn directly: even columns have 5 distinct bins (equal scores between bins and between
    features are common), odd ones 256; the label follows two columns with noise.  Nine rows are
    built so that a tree must split twice."""
    rs = np.random.RandomState(1000 * n + d)
    if n == 9:
        # three groups of three equal rows; every column orders the groups 0 < 1 < 2 or 2 < 1 < 0 and
        # the label is the middle group, so no single threshold purifies a node that holds all three
        grp = np.arange(9) // 3
        v = np.sort(np.stack([rs.permutation(256)[:3] for _ in range(d)]), axis=1)
        v = np.where(rs.rand(d, 1) < 0.5, v, v[:, ::-1])
        return np.ascontiguousarray(v[:, grp].T.astype(np.uint8)), (grp == 1).astype(np.int32)
    Xb = rs.randint(0, 256, size=(n, d)).astype(np.uint8)
    Xb[:, ::2] = 40 * rs.randint(0, 5, size=Xb[:, ::2].shape)
    y = ((Xb[:, 0] >= 80).astype(int) + (Xb[:, d - 1] >= 128) + (rs.rand(n) < 0.2)) & 1
    return np.ascontiguousarray(Xb), y.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _tie_table(n):
    """d = 11: columns 2 i and 2 i + 1 are identical (i < 5), each with 3 distinct bins; column 10 is
    constant.  Whichever of a pair is visited first must be the one a split names."""
    rs = np.random.RandomState(77 + n)
    base = 60 * rs.randint(0, 3, size=(n, 5))
    Xb = np.zeros((n, 11), np.uint8)
    Xb[:, 0:10:2] = base
    Xb[:, 1:10:2] = base
    Xb[:, 10] = 9
    y = ((base[:, 0] >= 60).astype(int) + (base[:, 3] >= 120) + (rs.rand(n) < 0.25)) & 1
    return np.ascontiguousarray(Xb), y.astype(np.int32)


def _specs(d, criterion, bootstrap=1):
    combos = [(k, m) for k in _max_features(d) for m in MSL]
    specs = forest_ops.make_specs(PER * len(combos))
    for t, s in enumerate(specs):
        k, m = combos[t // PER]
        s["seed"] = 4242 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = m
        s["max_features"] = k
        s["bootstrap"] = bootstrap
        s["criterion"] = criterion
        s["pois_cdf"] = native.poisson_cdf_table(1.0)
    return specs, combos


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


def _compare(Xb_cpu, ycls, criterion, bootstrap=1):
    n, d = Xb_cpu.shape
    specs, combos = _specs(d, criterion, bootstrap)
    T = len(specs)
    roles = np.ones((1, n), np.uint8)
    dev = torch.device("cuda:0")
    Xb = torch.from_numpy(Xb_cpu).to(dev)
    g = forest_ops.build_gpu(Xb, torch.from_numpy(ycls).to(dev), None, torch.from_numpy(roles).to(dev), specs, 2, False,
                             forest_ops.ForestTiers(**TIERS))
    c = forest_ops.build_cpu(Xb_cpu, ycls, None, roles, specs, 2, False)
    assert g.stats["tier_nodes"][0] > 0                       # subtree roots
    gc = _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), T)
    cc = _canon(c.nodes, c.vals, T)
    # the host builder grows every tree, and in every (max_features, min_samples_leaf) group that can
    # split twice (9 rows with 4 per leaf cannot) some tree splits below its root
    for ci, (k, m) in enumerate(combos):
        sizes = [len(cc[t]) for t in range(ci * PER, (ci + 1) * PER)]
        assert min(sizes) >= 1
        if n >= 4 * m:
            assert max(sizes) >= 5, (n, d, k, m, sizes)
    assert gc == cc
    return c, specs


@pytest.mark.parametrize("criterion", [forest_ops.GINI, forest_ops.ENTROPY])
@pytest.mark.parametrize("d", [3, 11, 100])
@pytest.mark.parametrize("n", [9, 33, 64, 200])
def test_sub_post_matches_host(n, d, criterion):
    Xb, y = _table(n, d)
    _compare(Xb, y, criterion)


def _cpu():
    lib = native.cpu_lib()
    lib.dml_node_root_key.restype = ctypes.c_uint64
    lib.dml_node_root_key.argtypes = [ctypes.c_uint64]
    lib.dml_node_child_key.restype = ctypes.c_uint64
    lib.dml_node_child_key.argtypes = [ctypes.c_uint64, ctypes.c_int32]
    lib.dml_node_visit_order.restype = None
    lib.dml_node_visit_order.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p]
    return lib




def _seg_stride(cnt):
    """Visiting positions p and p + S share one packed sort (low and high key half) in a subtree node
    of cnt rows: the one-feature path (33..64 rows) pairs 2 i and 2 i + 1, a segmented pass has
    S = 64 / WD segments of WD = 8, 16 or 32 lanes."""
    return 1 if cnt > 32 else 64 // (8 if cnt <= 8 else 16 if cnt <= 16 else 32)


def _shares_sort(a, b, S):
    """a in a low half, b in the high half of the same sort and segment."""
    return a // (2 * S) == b // (2 * S) and (a // S) % 2 == 0 and b == a + S


@pytest.mark.parametrize("n", [33, 64, 200])
def test_sub_post_ties_between_key_halves(n):
    """Identical columns: the split names the twin visited first.  The trees keep every row (no
    bootstrap), so a node's row count and with it the path and segment width it took are known from
    the host's tree: among its splits there are nodes whose winning pair lies in the two halves of
    ONE packed sort, in the one-feature path and in the segmented path, so the low-half-wins rule of
    the shared reduction is what is being compared."""
    Xb, y = _tie_table(n)
    c, specs = _compare(Xb, y, forest_ops.GINI, bootstrap=0)
    lib = _cpu()
    d = Xb.shape[1]
    order = np.zeros(d, np.int32)
    shared = {"one-feature": 0, "segmented": 0}
    for t in range(len(specs)):
        stack = [(t, np.arange(n), lib.dml_node_root_key(int(specs[t]["seed"])))]
        while stack:
            i, rows, key = stack.pop()
            s, l = int(c.nodes[i, 0]), int(c.nodes[i, 1])
            if s < 0:
                continue
            f = s // 256
            left = Xb[rows, f] <= (s % 256)
            stack.append((l, rows[left], lib.dml_node_child_key(key, 0)))
            stack.append((l + 1, rows[~left], lib.dml_node_child_key(key, 1)))
            if f >= 10:
                continue
            lib.dml_node_visit_order(key, d, order.ctypes.data)
            pos = {int(ff): p for p, ff in enumerate(order)}
            assert pos[f] < pos[f ^ 1], (t, i, f)                  # the earlier twin is named
            if len(rows) <= 64 and _shares_sort(pos[f], pos[f ^ 1], _seg_stride(len(rows))):
                shared["one-feature" if len(rows) > 32 else "segmented"] += 1
    assert shared["one-feature"] > 0 and shared["segmented"] > 0, shared


# Near ties: a node of n0 class-0 and n1 class-1 rows under integer class weights (p, q), and two
# two-bin features whose only thresholds put (a0, a1) and (b0, b1) rows of the classes on the left.
# The Gini proxies are the rationals
#   (p^2 l0^2 + q^2 l1^2) / (p l0 + q l1) + (p^2 r0^2 + q^2 r1^2) / (p r0 + q r1),
# found by a search over all pairs of thresholds of such nodes: they differ by less than 2^-30 of
# their value, the second is the greater, and the host's fp64 scores differ in the same direction.
# (Without class weights the proxies of a node of at most 64 unit-weight rows cannot come closer
# than about 2^-26 of their value: the class weights are what makes the denominators large.)
NEAR = {64: dict(cw=(1, 11), n0=5, n1=59, a=(1, 32), b=(2, 42), d=2),       # one-feature path
        32: dict(cw=(2, 57), n0=5, n1=27, a=(3, 25), b=(4, 7), d=4)}        # segmented path, S = 2


def _proxy_exact(p, q, n0, n1, l0, l1):
    from fractions import Fraction
    a0, a1, b0, b1 = p * l0, q * l1, p * (n0 - l0), q * (n1 - l1)
    return Fraction(a0 * a0 + a1 * a1, a0 + a1) + Fraction(b0 * b0 + b1 * b1, b0 + b1)


def _proxy_f64(p, q, n0, n1, l0, l1):
    """cls_proxy's operations in order, in float64 (no fused multiply-add)."""
    f = np.float64
    a0, a1 = f(l0) * f(p), f(l1) * f(q)
    b0, b1 = f(n0) * f(p) - a0, f(n1) * f(q) - a1
    lw, rw = a0 + a1, b0 + b1
    lsq, rsq = a0 * a0 + a1 * a1, b0 * b0 + b1 * b1
    return (lsq * rw + rsq * lw) / (lw * rw)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("n", [64, 32])
def test_sub_post_near_ties_between_key_halves(n, swap):
    """Two scores closer than 2^-30 of their value, one in each half of one packed sort, in both
    orders (the greater in the low half, the greater in the high half): the root must name the
    greater, as on the host.  Class weights send the build to the generic (FC = -1) kernel's Gini
    code."""
    from fractions import Fraction
    case = NEAR[n]
    p, q = case["cw"]
    n0, n1, d = case["n0"], case["n1"], case["d"]
    assert n0 + n1 == n
    ea, eb = _proxy_exact(p, q, n0, n1, *case["a"]), _proxy_exact(p, q, n0, n1, *case["b"])
    ga, gb = _proxy_f64(p, q, n0, n1, *case["a"]), _proxy_f64(p, q, n0, n1, *case["b"])
    assert ea < eb and (eb - ea) / eb < Fraction(1, 2**30)
    assert ga < gb                                               # fp64 separates them, the same way
    col_a, col_b = (d - 1, 0) if swap else (0, d - 1)
    y = np.concatenate([np.zeros(n0, np.int32), np.ones(n1, np.int32)])
    Xb = np.full((n, d), 9, np.uint8)                            # the other columns are constant
    for col, (l0, l1) in ((col_a, case["a"]), (col_b, case["b"])):
        Xb[:, col] = 200
        Xb[:l0, col] = 10
        Xb[n0:n0 + l1, col] = 10
    T = 32
    specs = forest_ops.make_specs(T)
    for t, s in enumerate(specs):
        s["seed"] = 31337 + t
        s["split"] = 0
        s["fit"] = 0
        s["max_depth"] = 2**31 - 1
        s["min_samples_split"] = 2
        s["min_samples_leaf"] = 1
        s["max_features"] = d
        s["bootstrap"] = 0
        s["criterion"] = forest_ops.GINI
        s["cw_mode"] = 1
    cw = np.tile(np.array([[p, q]], np.float64), (T, 1))
    roles = np.ones((1, n), np.uint8)
    c = forest_ops.build_cpu(Xb, y, None, roles, specs, 2, False, cw=cw.copy())
    # the host: every root splits on the column of the greater score; and over the trees that
    # column is met in the low half with the other in the high half of the same sort, and the
    # other way round
    lib = _cpu()
    order = np.zeros(d, np.int32)
    S = _seg_stride(n)
    greater_low = greater_high = 0
    for t in range(T):
        assert int(c.nodes[t, 0]) // 256 == col_b, t
        lib.dml_node_visit_order(lib.dml_node_root_key(int(specs[t]["seed"])), d, order.ctypes.data)
        pos = {int(ff): pp for pp, ff in enumerate(order)}
        greater_low += _shares_sort(pos[col_b], pos[col_a], S)
        greater_high += _shares_sort(pos[col_a], pos[col_b], S)
    assert greater_low > 0 and greater_high > 0, (greater_low, greater_high)
    dev = torch.device("cuda:0")
    g = forest_ops.build_gpu(torch.from_numpy(Xb).to(dev), torch.from_numpy(y).to(dev), None, torch.from_numpy(roles).to(dev),
                             specs, 2, False, forest_ops.ForestTiers(**TIERS), cw=cw.copy())
    assert g.stats["tier_nodes"][0] > 0
    assert _canon(g.nodes.cpu().numpy(), g.vals.cpu().numpy(), T) == _canon(c.nodes, c.vals, T)

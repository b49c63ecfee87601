"""Inputs and the brute-force reference of the one-vs-one pair statistics (shared by
test_pair_rank.py and test_pair_rank_gpu.py; not a test module).  A case is (id, C, score kind,
fits), a fit being its entry count per class."""
import numpy as np

N_Y = 4096
CASES = [
    # a lone entry, then a wave cut short by one, a whole wave, a wave and one entry
    ("wave", 3, "softmax", [(1, 0, 0), (21, 21, 21), (22, 21, 21), (22, 22, 21)]),
    # a tile cut short by one, a whole tile, a tile and one entry (count, scatter and sort)
    ("tile-1", 3, "softmax", [(1365, 1365, 1365)]),
    ("tile", 3, "softmax", [(1366, 1365, 1365)]),
    ("tile+1", 3, "softmax", [(1366, 1366, 1365)]),
    # fits of different lengths in one call, the second without class 1
    ("absent", 4, "softmax", [(50, 60, 70, 20), (10, 0, 17, 10), (400, 300, 200, 100), (2, 1, 1, 1)]),
    # 8 score levels, column 1 all equal, column 2 a mix of -0.0 and +0.0
    ("ties", 5, "ties", [(60, 50, 40, 30, 20), (900, 800, 1000, 700, 600)]),
    # 17 * 64 * 64 = 69,632 segments and pair problems: more than one launch holds in grid y
    ("C64", 64, "softmax", [tuple(1 + (k + f) % 2 for k in range(64)) for f in range(17)]),
    # classes 0 and 2 are one tile each, and their first and last keys span more than 17,000 of class 1's sorted
    # keys: more than the reduce stages in LDS (test_pair_rank_gpu.py computes the windows and asserts it)
    ("window", 3, "softmax", [(100, 20000, 500)]),
]
IDS = [c[0] for c in CASES]


def build(case, seed=0):
    """(rows int32 [total], off int64 [F + 1], score float32 [total, C], y int32 [N_Y])."""
    _id, C, kind, fits = case
    rng = np.random.RandomState(seed + C)
    y = rng.randint(0, C, size=N_Y).astype(np.int32)
    rows = [rng.permutation(np.concatenate([rng.choice(np.nonzero(y == k)[0], size=m) for k, m in enumerate(f)]))
            for f in fits]
    off = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    rows = np.concatenate(rows).astype(np.int32)
    z = rng.normal(size=(rows.size, C)) + 1.2 * np.eye(C)[y[rows]]
    if kind == "softmax":   # rows sum to 1, as sklearn's roc_auc_score asks
        s = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    else:
        s = np.clip(np.floor(z * 2.0), -4, 3) / 2.0
        s[:, 1] = 0.25
        s[:, 2] = np.where(rng.rand(rows.size) < 0.5, -0.0, 0.0)
    return rows, off, s.astype(np.float32), y


def windows(score, t, C, tile):
    """For one fit (scores, classes of its entries): per ordered pair (c, l) and per tile of the sorted class-c
    scores of column c, the class-l scores between the tile's first and last score, as k_pair_reduce bounds it."""
    out = []
    for c in range(C):
        for l in range(C):
            a, b = np.sort(score[t == c, c]), np.sort(score[t == l, c])
            out += [int(np.searchsorted(b, a[min(i + tile, a.size) - 1], "right") - np.searchsorted(b, a[i], "left"))
                    for i in range(0, a.size if l != c else 0, tile)]
    return out


def brute_force(rows, off, score, y, C):
    """n int64 [F, C] and U2 int64 [F, C, C] by comparing every pair of entries in float64."""
    F = len(off) - 1
    n, u2 = np.zeros((F, C), dtype=np.int64), np.zeros((F, C, C), dtype=np.int64)
    for f in range(F):
        t = y[rows[off[f]:off[f + 1]]]
        s = (score[off[f]:off[f + 1]] + np.float32(0.0)).astype(np.float64)
        n[f] = np.bincount(t, minlength=C)
        for c in range(C):
            for l in range(C):
                if l != c:
                    a, b = s[t == c, c][:, None], s[t == l, c][None, :]
                    u2[f, c, l] = 2 * int((a > b).sum()) + int((a == b).sum())
    return n, u2

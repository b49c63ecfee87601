"""Synthetic inputs for the segmented sort and the rank / probability statistics (shared by
test_rank_stats.py and test_rank_stats_gpu.py; not a test module).

Segment and fit lengths: 0, 1, 2, 63, 64, 65, 257, tile - 1, tile, tile + 1 and 2 * tile + 3 -- an
empty one, parts of a wave, a whole wave, more than one wave, a block's tile cut short by one, a
whole tile, a tile and one key, and three tiles with the last cut short.  Problem cases add three
fits: one without a positive, one without a negative, and one with one of each.  Row ids are
scattered over a 5,000-row target vector."""
import numpy as np

N_Y = 5000
KEY_KINDS = ("random", "equal", "top_byte", "low_byte", "sorted", "reversed")
SCORE_KINDS = ("grid", "continuous", "zeros", "inf", "denormal")


def lens(tile):
    return (0, 1, 2, 63, 64, 65, 257, tile - 1, tile, tile + 1, 2 * tile + 3)


def sort_case(tile, kind, seed=0):
    """(keys uint32 [total], seg_off int64 [S + 1])."""
    rng = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(lens(tile))]).astype(np.int64)
    n = int(off[-1])
    if kind == "random":
        keys = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    elif kind == "equal":
        keys = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    elif kind == "top_byte":
        keys = (rng.randint(0, 256, size=n).astype(np.uint32) << 24) | np.uint32(0x00ABCDEF)
    elif kind == "low_byte":
        keys = rng.randint(0, 256, size=n).astype(np.uint32) | np.uint32(0x12345600)
    else:
        keys = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        for s in range(len(off) - 1):
            seg = np.sort(keys[off[s]:off[s + 1]])
            keys[off[s]:off[s + 1]] = seg if kind == "sorted" else seg[::-1]
    return keys, off


def sorted_segments(keys, off):
    out = keys.copy()
    for s in range(len(off) - 1):
        out[off[s]:off[s + 1]] = np.sort(keys[off[s]:off[s + 1]])
    return out


def _scores(kind, y01, rng):
    """float32 scores of entries whose 0/1 labels are y01, correlated with the label."""
    m = y01.size
    if kind == "grid":   # forest-like: multiples of 1/50, heavy ties
        return (np.clip(rng.binomial(50, 0.35 + 0.3 * y01), 0, 50) / 50.0).astype(np.float32)
    if kind == "continuous":
        return (rng.normal(size=m) + 0.8 * y01).astype(np.float32)
    if kind == "zeros":   # mixed sign with planted +0.0 and -0.0
        s = (rng.normal(size=m) + 0.5 * y01).astype(np.float32)
        z = rng.rand(m)
        s[z < 0.2] = 0.0
        s[z < 0.1] = -0.0
        return s
    if kind == "inf":
        s = (rng.normal(size=m) + 0.5 * y01).astype(np.float32)
        z = rng.rand(m)
        s[z < 0.1] = np.inf
        s[z < 0.05] = -np.inf
        return s
    assert kind == "denormal"   # multiples of the smallest float32 denormal, both signs
    return (rng.randint(-40, 41, size=m) + 8 * y01).astype(np.float32) * np.float32(1.4e-45)


def _fits(tile, y, rng, cls_a=0, cls_b=1):
    """Row ids per fit: the lengths of ``lens``, then no ``cls_b``, only ``cls_b``, one of each."""
    rows = [rng.randint(0, N_Y, size=m).astype(np.int32) for m in lens(tile)]
    ia, ib = np.nonzero(y != cls_b)[0], np.nonzero(y == cls_b)[0]
    rows.append(rng.choice(ia, size=40).astype(np.int32))
    rows.append(rng.choice(ib, size=40).astype(np.int32))
    rows.append(np.array([rng.choice(np.nonzero(y == cls_a)[0]), rng.choice(ib)], dtype=np.int32))
    off = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    return np.concatenate(rows), off


def binary_case(tile, kind, seed=0, prevalence=0.4):
    """K = 1: (rows int32, off int64, score float32 [total], y int32 [N_Y])."""
    rng = np.random.RandomState(seed)
    y = (rng.rand(N_Y) < prevalence).astype(np.int32)
    rows, off = _fits(tile, y, rng)
    return rows, off, _scores(kind, y[rows], rng), y


def proba_case(tile, C, kind, seed=0):
    """K = C: (rows, off, proba float32 [total, C], y int32 [N_Y]).  ``grid``: class counts of 50
    draws / 50 (ties, exact zeros and ones); ``continuous``: a normalised exponential."""
    rng = np.random.RandomState(seed)
    y = rng.randint(0, C, size=N_Y).astype(np.int32)
    rows, off = _fits(tile, y, rng, cls_a=0, cls_b=C - 1)
    t = y[rows]
    w = np.full((t.size, C), 1.0)
    w[np.arange(t.size), t] += 0.6 * C
    w /= w.sum(1, keepdims=True)
    if kind == "grid":
        p = np.stack([rng.multinomial(50, wi) for wi in w]).astype(np.float64) / 50.0
    else:
        p = rng.gamma(w * 4.0 + 0.05)
        p /= p.sum(1, keepdims=True)
    return rows, off, p.astype(np.float32), y

"""The segmented binary Gini split search (forest.hip eval_gini_seg<2 / 4>: two or four features
per wave pass) against the one-feature routine (eval_gini_pf) through dml_test_eval_seg: every
output of every feature -- gain, bin, non-constant flag, the left child's channel sums -- must
be the same bit pattern, and both must clear the histogram words they read.  The one-feature
routine's bin and gain are checked against a float64 sweep in numpy as well, so the two cannot
be wrong together."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu

F = 8   # kEvalSegTestFeats: features per block of the test kernel


def _pack(w0, w1, rows, word64):
    w0, w1, rows = (np.asarray(a, dtype=np.uint64) for a in (w0, w1, rows))
    if word64:
        assert w0.max() < (1 << 21) and w1.max() < (1 << 21) and rows.max() < (1 << 22)
        return w0 | (w1 << np.uint64(21)) | (rows << np.uint64(42))
    assert w0.max() < (1 << 12) and w1.max() < (1 << 12) and rows.max() < (1 << 8)
    return (w0 | (w1 << np.uint64(12)) | (rows << np.uint64(24))).astype(np.uint32)


def _hist(bins, cls, w):
    """(3, 256) integer sums of rows given as (bin, class, weight)."""
    h = np.zeros((3, 256), dtype=np.int64)
    np.add.at(h[0], bins[cls == 0], w[cls == 0])
    np.add.at(h[1], bins[cls == 1], w[cls == 1])
    np.add.at(h[2], bins, 1)
    return h


def _random_hist(rs, nrows, nbins):
    """nrows rows with weights 1..12 over nbins distinct random bins."""
    support = rs.choice(256, size=nbins, replace=False)
    bins = support[rs.randint(0, nbins, size=nrows)]
    cls = (rs.rand(nrows) < 0.35 + 0.3 * (bins > np.median(support))).astype(np.int64)
    return _hist(bins, cls, rs.randint(1, 13, size=nrows))


def _one_bin(rs):
    n = int(rs.randint(65, 256))
    return _hist(np.full(n, int(rs.randint(0, 256))), rs.randint(0, 2, size=n), rs.randint(1, 13, size=n))


def _last_bins(rs):
    n = int(rs.randint(65, 256))
    return _hist(254 + rs.randint(0, 2, size=n), rs.randint(0, 2, size=n), rs.randint(1, 13, size=n))


def _symmetric(b1, b2, b3, a, c):
    """(a, 0) | (c, c) | (0, a): the cuts after b1 and after b2 score the same doubles."""
    h = np.zeros((3, 256), dtype=np.int64)
    h[:, b1] = (a, 0, a)
    h[:, b2] = (c, c, 2 * c)
    h[:, b3] = (0, a, a)
    return h


def _two_rows_aside(rs):
    """Non-constant, but the only cut leaves 2 rows on the left: nothing admissible from
    min_samples_leaf = 3 on."""
    n = int(rs.randint(65, 256))
    bins = np.full(n, 9)
    bins[:2] = 5
    return _hist(bins, rs.randint(0, 2, size=n), rs.randint(1, 13, size=n))


@functools.lru_cache(maxsize=None)
def _blocks(word64, nfeat):
    """The cases of one launch, (nblocks, nfeat, 3, 256) integer histograms, and the block
    index ranges by case name."""
    rs = np.random.RandomState(1000 * nfeat + int(word64))
    blocks, names = [], {}

    def add(name, feats):
        names.setdefault(name, []).append(len(blocks))
        blocks.append(np.stack(feats))

    for _ in range(4):   # sparse: 65..255 rows on few bins, so most lanes hold no candidate
        add("sparse", [_random_hist(rs, int(rs.randint(65, 256)), int(rs.randint(2, 40))) for _ in range(nfeat)])
    add("sparse", [_random_hist(rs, 255, 256) for _ in range(nfeat)])
    if word64:
        for _ in range(2):   # dense: candidates in every lane, several per lane
            add("dense", [_random_hist(rs, int(rs.randint(256, 4001)), 256) for _ in range(nfeat)])
    add("one_bin", [_one_bin(rs) for _ in range(nfeat)])
    add("last_bins", [_last_bins(rs) for _ in range(nfeat)])
    # equal-gain pairs inside one lane, in neighbouring lanes, across 16- and 32-lane boundaries
    sym = [(8, 9, 200), (10, 100, 200), (3, 4, 5), (63, 64, 65), (127, 128, 129), (15, 16, 254), (0, 31, 32),
           (120, 135, 250)]
    add("symmetric", [_symmetric(*sym[(f + nfeat) % len(sym)], a=7 + f, c=3 + 2 * f) for f in range(nfeat)])
    same = _random_hist(rs, 200, 30)
    add("same", [same for _ in range(nfeat)])
    # features without an admissible candidate beside features with candidates
    mixed = [_one_bin, _two_rows_aside]
    add("mixed", [mixed[(f // 2) % 2](rs) if f % 2 == 0 else _random_hist(rs, 150, 20) for f in range(nfeat)])
    add("mixed", [mixed[(f // 2) % 2](rs) if f % 2 == 1 else _random_hist(rs, 150, 20) for f in range(nfeat)])
    return np.stack(blocks), names


def _run(h, word64, nseg, msl, mwl=0.0, cw0=1.0, cw1=1.0):
    """Both output sets of every block: dict of (nblocks, 2, nfeat[, 3]) arrays."""
    lib = native.hip_lib()
    nb, nfeat = h.shape[:2]
    words = _pack(h[:, :, 0], h[:, :, 1], h[:, :, 2], word64)
    wd = torch.from_numpy(np.ascontiguousarray(words).view(np.int64 if word64 else np.int32)).cuda()
    outd = torch.full((nb, 2, F, 4), float("nan"), dtype=torch.float64, device="cuda")
    outi = torch.full((nb, 2, F, 3), -7, dtype=torch.int32, device="cuda")
    rc = lib.dml_test_eval_seg(ctypes.c_void_p(wd.data_ptr()), int(word64), nfeat, nseg, msl, float(mwl), float(cw0),
                               float(cw1), ctypes.c_void_p(outd.data_ptr()), ctypes.c_void_p(outi.data_ptr()), nb, None)
    assert rc == 0
    torch.cuda.synchronize()
    d, i = outd.cpu().numpy()[:, :, :nfeat], outi.cpu().numpy()[:, :, :nfeat]
    return dict(gain=d[..., 0], left=d[..., 1:], bin=i[..., 0], nc=i[..., 1], dirty=i[..., 2])


def _reference(h, msl, mwl, cw0, cw1):
    """Float64 sweep of one feature: (gain, bin, nc, left) by the one-feature routine's rules."""
    c = np.cumsum(h, axis=1)
    t = c[:, 255]
    l0, l1, rl = c[0] * cw0, c[1] * cw1, c[2]
    r0, r1, rr = t[0] * cw0 - l0, t[1] * cw1 - l1, t[2] - rl
    ok = (h[2] > 0) & (np.arange(256) != 255) & (rl >= msl) & (rr >= msl)
    if mwl > 0.0:
        ok &= ~((l0 + l1 < mwl) | (r0 + r1 < mwl))
    nc = int(np.any((rl > 0) & (rr > 0)))
    if not ok.any():
        return -np.inf, -1, nc, (0.0, 0.0, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = ((l0 * l0 + l1 * l1) * (r0 + r1) + (r0 * r0 + r1 * r1) * (l0 + l1)) / ((l0 + l1) * (r0 + r1))
    g = np.where(ok, g, -np.inf)
    b = int(np.argmax(g))   # the first maximum: lowest bin
    return float(g[b]), b, nc, (float(l0[b]), float(l1[b]), float(rl[b]))


def _check(h, out, msl, mwl=0.0, cw0=1.0, cw1=1.0):
    one = {k: v[:, 0] for k, v in out.items()}
    seg = {k: v[:, 1] for k, v in out.items()}
    assert not one["dirty"].any() and not seg["dirty"].any()          # zero_after cleared every word read
    assert np.array_equal(one["bin"], seg["bin"])
    assert np.array_equal(one["nc"], seg["nc"])
    assert np.array_equal(one["gain"].view(np.int64), seg["gain"].view(np.int64))
    assert np.array_equal(one["left"].view(np.int64), seg["left"].view(np.int64))
    for b in range(h.shape[0]):
        for f in range(h.shape[1]):
            g, bb, nc, left = _reference(h[b, f], msl, mwl, cw0, cw1)
            assert (one["bin"][b, f], one["nc"][b, f]) == (bb, nc), (b, f)
            assert tuple(one["left"][b, f]) == left, (b, f)
            # integer sums times the class weights: every term of the score is exact or rounded
            # once the same way; a few ulps cover the division and a contracted multiply-add
            assert one["gain"][b, f] == g or abs(one["gain"][b, f] - g) <= 1e-15 * abs(g), (b, f)


def _skip_if_off():
    if native.hip_lib().dml_forest_eval_seg() == 0:
        pytest.skip("library built with DML_EVAL_SEG=0")


@pytest.mark.parametrize("msl", [1, 3])
@pytest.mark.parametrize("nseg", [2, 4])
@pytest.mark.parametrize("word64", [False, True])
def test_segmented_matches_one_feature(word64, nseg, msl):
    _skip_if_off()
    for nfeat in range(1, F + 1):
        h, names = _blocks(word64, nfeat)
        out = _run(h, word64, nseg, msl)
        _check(h, out, msl)
        one = {k: v[:, 0] for k, v in out.items()}
        for b in names["one_bin"]:
            assert (one["nc"][b] == 0).all() and (one["bin"][b] == -1).all()
        for b in names["last_bins"]:   # bin 255 is no candidate: the cut is after 254 or there is none
            assert np.isin(one["bin"][b], (-1, 254)).all()
        for b in names["symmetric"]:   # two equal doubles: the lower bin
            lo = [int(np.flatnonzero(h[b, f, 2])[0]) for f in range(nfeat)]
            assert list(one["bin"][b]) == lo
        for b in names["same"]:
            for k in ("gain", "bin", "nc"):
                assert (out[k][b, 1] == out[k][b, 1, 0]).all()
        if msl == 3:
            for b in names["mixed"]:
                two = [f for f in range(nfeat) if h[b, f, 2, 5] == 2 and h[b, f, 2, 9] > 0 and h[b, f, 2].sum() == h[b, f, 2, 5] + h[b, f, 2, 9]]
                for f in two:
                    assert one["bin"][b, f] == -1 and one["nc"][b, f] == 1


@pytest.mark.parametrize("msl", [1, 3])
@pytest.mark.parametrize("nseg", [2, 4])
@pytest.mark.parametrize("word64", [False, True])
def test_segmented_class_weights_and_min_weight_leaf(word64, nseg, msl):
    """The generic-criterion kernels' form: class weights 0.5 and 3 multiply the integer sums and
    min_weight_leaf rejects light sides (same doubles as the one-feature routine)."""
    _skip_if_off()
    for nfeat in range(1, F + 1):
        h, _ = _blocks(word64, nfeat)
        out = _run(h, word64, nseg, msl, mwl=40.0, cw0=0.5, cw1=3.0)
        _check(h, out, msl, mwl=40.0, cw0=0.5, cw1=3.0)

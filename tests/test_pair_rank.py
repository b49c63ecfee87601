"""The one-vs-one pair statistics on the host (docs/RANK_SCORES.md): the twin of
``dml_pair_rank_stats`` against a brute-force comparison of every pair of entries, and
``score_from_pair_stats`` against ``scoring.score`` (the same double) and sklearn's
``roc_auc_score(multi_class="ovo")`` (1e-12) for roc_auc_ovo and roc_auc_ovo_weighted."""
import numpy as np
import pytest
import torch

import pair_rank_cases as pc
from cs230_distributed_machine_learning_amd.search import scoring


def _same(a, b):
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_twin_counts_and_scores(case):
    from sklearn.metrics import roc_auc_score

    C = case[1]
    rows, off, s, y = pc.build(case)
    tr, ts, ty = torch.from_numpy(rows), torch.from_numpy(s), torch.from_numpy(y)
    st = scoring.pair_rank_statistics(tr, off, ts, ty, C)
    n, u2 = pc.brute_force(rows, off, s, y, C)
    np.testing.assert_array_equal(st["n"], n)
    np.testing.assert_array_equal(st["u2"].astype(np.int64), u2)
    # the references cost 4,032 argsorts per fit at C = 64: the counts above cover all its fits, the scores one
    for f in (range(len(off) - 1) if C < 64 else [len(off) - 2]):
        yf, sf = y[rows[off[f]:off[f + 1]]], s[off[f]:off[f + 1]]
        for name, avg in (("roc_auc_ovo", "macro"), ("roc_auc_ovo_weighted", "weighted")):
            got = scoring.score_from_pair_stats(name, st[f], C)
            ref = scoring.score(name, torch.from_numpy(yf), torch.from_numpy(yf), C, torch.from_numpy(sf))
            assert _same(got, ref), (name, f, got, ref)
            assert (got != got) == bool((n[f] == 0).any())
            if case[2] == "softmax" and got == got:
                sk = roc_auc_score(yf, sf.astype(np.float64), multi_class="ovo", average=avg, labels=np.arange(C))
                assert abs(got - sk) <= 1e-12, (name, f, got, sk)


def test_bad_entries_raise_and_leave_the_other_fits_alone():
    case = pc.CASES[4]
    rows, off, s, y = pc.build(case)
    ty = torch.from_numpy(y)
    clean = scoring.pair_rank_statistics(torch.from_numpy(rows), off, torch.from_numpy(s), ty, 4)
    bad_s, bad_r = s.copy(), rows.copy()
    bad_s[off[2] + 5, 3] = np.nan
    bad_r[off[3] - 1] = pc.N_Y
    with pytest.raises(ValueError, match="pair_rank_statistics: fit 2 has 1 "):
        scoring.pair_rank_statistics(torch.from_numpy(rows), off, torch.from_numpy(bad_s), ty, 4)
    with pytest.raises(ValueError, match="pair_rank_statistics: fit 2 has 1 "):
        scoring.pair_rank_statistics(torch.from_numpy(bad_r), off, torch.from_numpy(s), ty, 4)
    keep = np.r_[0:off[2], off[3]:off[4]]   # the call without fit 2
    off2 = np.array([0, off[1], off[2], off[2] + off[4] - off[3]])
    rest = scoring.pair_rank_statistics(torch.from_numpy(bad_r[keep]), off2, torch.from_numpy(bad_s[keep]), ty, 4)
    assert rest.tobytes() == clean[[0, 1, 3]].tobytes()
    with pytest.raises(ValueError, match="not computable"):
        scoring.score_from_pair_stats("roc_auc_ovr", clean[0], 4)

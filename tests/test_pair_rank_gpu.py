"""``dml_pair_rank_stats`` (csrc/kernels/rank_stats.hip) on the MI355X against its host twin: the
class counts, the pair counts U2 and the bad counts are integers, compared bit for bit on the cases
of tests/pair_rank_cases.py; then ``_rank_proba_scores`` for roc_auc_ovo* against
``scoring.score`` on the same device tensors (docs/RANK_SCORES.md)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pair_rank_cases as pc
from cs230_distributed_machine_learning_amd.search import scoring
from cs230_distributed_machine_learning_amd.utils import native

pytestmark = pytest.mark.gpu


def _both(rows, off, s, y, C):
    t = [torch.from_numpy(a) for a in (rows, s, y)]
    return (scoring.pair_rank_statistics(t[0], off, t[1], t[2], C),
            lambda: scoring.pair_rank_statistics(t[0].cuda(), off, t[1].cuda(), t[2].cuda(), C))


@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_kernel_statistics_equal_the_twin(case, monkeypatch):
    C = case[1]
    rows, off, s, y = pc.build(case)
    host, run = _both(rows, off, s, y, C)
    dev = run()
    np.testing.assert_array_equal(dev["n"], host["n"])
    np.testing.assert_array_equal(dev["u2"], host["u2"])
    assert run().tobytes() == dev.tobytes()   # integer atomics only: the same bytes every run
    if case[0] == "window":   # its one fit has tiles on both sides of the LDS window: both search branches ran
        lib = native.hip_lib()
        w = pc.windows(s, y[rows], C, int(lib.dml_rank_stats_tile()))
        print("windows", sorted(w), "LDS holds", int(lib.dml_pair_rank_window()))
        assert min(w) <= int(lib.dml_pair_rank_window()) < max(w)
    if case[0] == "absent":
        monkeypatch.setattr(scoring, "RANK_CHUNK_KEYS", 2000)   # several chunks of fits, the long fit alone
        assert run().tobytes() == host.tobytes()


def test_bad_entries_are_counted_like_the_twin():
    rows, off, s, y = pc.build(pc.CASES[4])
    rows, s = rows.copy(), s.copy()
    s[off[2] + 5, 3] = np.nan
    rows[off[1] - 1] = -3
    msgs = []
    for dev in ("cpu", "cuda"):
        t = [torch.from_numpy(a).to(dev) for a in (rows, s, y)]
        with pytest.raises(ValueError, match="pair_rank_statistics: fit 0 has 1 ") as e1:
            scoring.pair_rank_statistics(t[0], off, t[1], t[2], 4)
        clean = torch.from_numpy(np.where(rows < 0, 0, rows)).to(dev)
        with pytest.raises(ValueError, match="pair_rank_statistics: fit 2 has 1 ") as e2:
            scoring.pair_rank_statistics(clean, off, t[1], t[2], 4)
        msgs.append((str(e1.value), str(e2.value)))
    assert msgs[0] == msgs[1]
    keep = np.r_[off[1]:off[2], off[3]:off[4]]   # the call without the two fits: the others' results stand
    off2 = np.array([0, off[2] - off[1], off[2] - off[1] + off[4] - off[3]])
    host, run = _both(*pc.build(pc.CASES[4]), 4)
    got = scoring.pair_rank_statistics(torch.from_numpy(rows[keep]).cuda(), off2, torch.from_numpy(s[keep]).cuda(),
                                       torch.from_numpy(y).cuda(), 4)
    assert got.tobytes() == host[[1, 3]].tobytes()


def test_rank_proba_scores_serves_ovo_with_the_bits_of_score():
    from cs230_distributed_machine_learning_amd.engine import executor

    rows, off, s, y = pc.build(pc.CASES[4])
    F = len(off) - 1
    ty = torch.from_numpy(y).cuda()
    data = SimpleNamespace(n_classes=4, y_cls=ty, is_row_shard=False,
                           test_rows=[torch.from_numpy(rows[off[f]:off[f + 1]]).cuda() for f in range(F)])
    tasks = [SimpleNamespace(task_id=10 + f, split=f) for f in range(F)]
    outputs = {10 + f: SimpleNamespace(error=None, decision=None, proba=torch.from_numpy(s[off[f]:off[f + 1]]).cuda())
               for f in range(F)}
    outputs[13].proba = outputs[13].proba.double()   # float64 probabilities stay per fit
    got = executor._rank_proba_scores(data, tasks, outputs, list(scoring.PAIR_SCORERS), True)
    assert sorted(got) == [10, 11, 12]
    for f in range(3):
        yf = ty[data.test_rows[f].long()]
        for name in scoring.PAIR_SCORERS:
            ref = scoring.score(name, yf, yf, 4, outputs[10 + f].proba)
            assert got[10 + f][name] == ref or (f == 1 and ref != ref and got[11][name] != got[11][name]), (name, f)

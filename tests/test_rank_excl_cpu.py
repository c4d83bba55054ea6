"""CPU tests of the filtered full-ranking evaluation: the per-user seen-items CSR (tlsan_amd.input.seen_items_csr) against
a plain-Python construction on the committed sets, the metrics of a rank histogram against a direct float64 computation,
and the driver's flags."""
import os

import numpy as np
import pytest

from tlsan_amd.input import load_packed, seen_items_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_seen(train_set, n_users):
    """One set per user, sample by sample."""
    seen = [set() for _ in range(n_users)]
    for k in range(len(train_set.u)):
        s = seen[int(train_set.u[k])]
        s.update(int(x) for x in train_set.hist[train_set.hist_off[k]:train_set.hist_off[k + 1]])
        s.update(int(x) for x in train_set.sess[train_set.sess_off[k]:train_set.sess_off[k + 1]])
        if int(train_set.label[k]) == 1:
            s.add(int(train_set.target[k]))
    return seen


# (set, longest list, test labels inside their user's list, test rows whose input is not inside the list)
@pytest.mark.parametrize("name,max_len,labels_inside,rows_outside", [("clothing", 49, 1719, 386),
                                                                    ("digital_music", 89, 1517, 189)])
def test_seen_items_csr_equals_sets_per_user(name, max_len, labels_inside, rows_outside):
    train_set, test_set, (U, I, _), _ = load_packed(os.path.join(ROOT, "tests", "golden", "packed_%s.npz" % name))
    off, ids = seen_items_csr(train_set, U)
    want = _plain_seen(train_set, U)
    assert off.shape == (U + 1,) and off[0] == 0 and off[-1] == len(ids)
    assert ids.min() >= 0 and ids.max() < I
    for u in range(U):
        lst = ids[off[u]:off[u + 1]].tolist()
        assert lst == sorted(want[u]), u                 # sorted and distinct, the same items
        assert len(lst) > 0, u                           # no user is empty
    ln = np.diff(off)
    assert ln.min() == 3 and ln.max() == max_len
    inside = sum(int(test_set.pos[k]) in want[int(test_set.u[k])] for k in range(len(test_set.u)))
    assert inside == labels_inside
    outside = 0
    for k in range(len(test_set.u)):
        row = set(test_set.hist[test_set.hist_off[k]:test_set.hist_off[k + 1]].tolist()) | \
            set(test_set.sess[test_set.sess_off[k]:test_set.sess_off[k + 1]].tolist())
        outside += not row <= want[int(test_set.u[k])]
    assert outside == rows_outside


def test_seen_items_csr_small_cases():
    from tlsan_amd.input import PackedSet
    samples = [(2, [5, 3, 5], [9], [1.0, 0.5, 0.2], 7, 1, 0), (0, [], [4, 4], [], 6, 0, 1), (2, [1], [], [1.0], 8, 0, 0)]
    off, ids = seen_items_csr(PackedSet.from_samples(samples), 4)
    assert off.tolist() == [0, 1, 1, 6, 6]               # users 1 and 3 have no sample: empty lists
    assert ids.tolist() == [4, 1, 3, 5, 7, 9]            # target 6 / 8 with label 0 are not interactions
    with pytest.raises(ValueError):
        seen_items_csr(PackedSet.from_samples(samples), 2)
    test = PackedSet.from_samples([(0, [1], [2], [1.0], (3, 4), 0)])
    with pytest.raises(ValueError):
        seen_items_csr(test, 1)


def _direct(ranks, ks):
    r = np.asarray(ranks, np.float64)
    out = {}
    for k in ks:
        out["HR@%d" % k] = float((r < k).sum()) / len(r)
    for k in ks:
        out["NDCG@%d" % k] = float(np.where(r < k, 1.0 / np.log2(r + 2.0), 0.0).sum()) / len(r)
    out["MRR"] = float((1.0 / (r + 1.0)).sum()) / len(r)
    return out


def test_full_ranking_metrics_from_histogram():
    from tlsan_amd.model import SAMPLED_KS, full_ranking_metrics, metrics_from_histogram, rank_histogram
    rng = np.random.RandomState(5)
    I = 1723
    ranks = np.minimum(rng.geometric(0.01, 5000) - 1, I - 1)
    ranks[:40] = 0
    hist = rank_histogram(ranks, I - 1)
    assert hist.shape == (I,) and hist.sum() == 5000
    got = full_ranking_metrics(hist)
    want = _direct(ranks, SAMPLED_KS)
    assert list(got) == list(want)                       # HR@k, NDCG@k, MRR -- and no AUC_N
    for k in want:
        assert abs(got[k] - want[k]) < 1e-12, k
    assert got["HR@20"] >= got["HR@10"] >= got["HR@5"] >= got["HR@1"] > 0.0
    # histograms of any split of the rows add up: identical floats
    for cut in (1, 777, 4999):
        both = rank_histogram(ranks[:cut], I - 1) + rank_histogram(ranks[cut:], I - 1)
        assert full_ranking_metrics(both) == got
    # one implementation of the sums: the sampled metrics are these plus AUC_N
    sampled = metrics_from_histogram(hist, I - 1)
    assert {k: v for k, v in sampled.items() if k != "AUC_N"} == got and "AUC_N" in sampled
    with pytest.raises(ValueError):
        rank_histogram([-1, 3], I - 1)                   # a negative filtered rank is an error, not a bin


def test_driver_flags():
    from tlsan_amd import train as T
    a = T.parse(["--dataset", "x"])
    assert (a.eval_rank_exclude, a.recommend_exclude, a.eval_neg_exclude) == ("off", "history", "history")
    for mode in ("off", "none", "history", "seen"):
        assert T.parse(["--eval_rank_exclude", mode]).eval_rank_exclude == mode
    a = T.parse(["--recommend_exclude", "seen", "--eval_neg_exclude", "seen"])
    assert (a.recommend_exclude, a.eval_neg_exclude) == ("seen", "seen")
    with pytest.raises(SystemExit):
        T.parse(["--eval_rank_exclude", "all"])
    holder = object()
    assert T.exclude_arg("none", holder) is None and T.exclude_arg("history", holder) == "history"
    assert T.exclude_arg("seen", holder) is holder
    line = T.full_ranking_line("seen", {"HR@1": 0.25, "MRR": 0.5})
    assert line == "Full ranking (exclude=seen): HR@1 = 0.2500 MRR = 0.5000"

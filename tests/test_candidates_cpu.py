"""Candidate scoring and the sampled evaluation, the parts that need no GPU: the C ABI declares and exports the three
entry points, bad arguments are refused before the device is touched, a numpy restatement of the sampler's definition,
the metrics helper, and the driver's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.candidates_ref import reference_negatives, splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tlsan_score_candidates", "tlsan_candidate_ranks", "tlsan_sample_negatives")


def _lib():
    from tlsan_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from tlsan_amd.build import build
        build()
    return L, L.load()


def test_candidate_symbols_declared_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    declared = set(re.findall(r"\b(tlsan_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.EXPORTS, name
        assert hasattr(lib, name), name
    assert L.NEG_MAX == 1024
    assert lib.tlsan_abi_version() == 15


def test_candidate_bad_arguments_are_rejected_without_a_launch():
    L, lib = _lib()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused by the argument checks
    p = L.Params(*([fake.value] * 8))
    sc = lib.tlsan_score_candidates
    assert sc(None, C.byref(p), fake, 16, 4, fake, 1, 0, fake, None) == -1
    assert sc(C.byref(dims), None, fake, 16, 4, fake, 1, 0, fake, None) == -1
    assert sc(C.byref(dims), C.byref(p), None, 16, 4, fake, 1, 0, fake, None) == -1
    assert sc(C.byref(dims), C.byref(p), fake, 16, 4, None, 1, 0, fake, None) == -1
    assert sc(C.byref(dims), C.byref(p), fake, 16, 4, fake, 1, 0, None, None) == -1
    for B, Cn in ((0, 4), (16, 0), (-1, 4), (16, -3)):
        assert sc(C.byref(dims), C.byref(p), fake, B, Cn, fake, 1, 0, fake, None) == -1
        assert b"B and C must be >= 1" in lib.tlsan_last_error()
    assert sc(C.byref(dims), C.byref(p), fake, 16, 4, fake, 0, 0, fake, None) == -1           # id_mul
    assert sc(C.byref(dims), C.byref(p), fake, 16, 4, fake, 1, -1, fake, None) == -1          # id_add
    assert sc(C.byref(dims), C.byref(p), fake, 16, 4, fake, 1 << 24, 0, fake, None) == -1     # ids past int32
    assert sc(C.byref(dims), C.byref(p), fake, 1 << 16, 1 << 15, fake, 1, 0, fake, None) == -4   # B * C past int32
    bad = L.Dims(100, 200, 10, 96, 48, 48, 8, 10)
    assert sc(C.byref(bad), C.byref(p), fake, 16, 4, fake, 1, 0, fake, None) == -4
    assert b"unsupported" in lib.tlsan_last_error()

    cr = lib.tlsan_candidate_ranks
    assert cr(None, fake, 16, 4, fake, None) == -1
    assert cr(fake, None, 16, 4, fake, None) == -1
    assert cr(fake, fake, 16, 4, None, None) == -1
    assert cr(fake, fake, 0, 4, fake, None) == -1
    assert cr(fake, fake, 16, 0, fake, None) == -1

    sn = lib.tlsan_sample_negatives
    assert sn(100, None, 16, 10, 1234, 0, None, None, fake, None) == -1
    assert sn(100, fake, 16, 10, 1234, 0, None, None, None, None) == -1
    assert sn(100, fake, 0, 10, 1234, 0, None, None, fake, None) == -1
    assert sn(0, fake, 16, 10, 1234, 0, None, None, fake, None) == -1
    for n in (0, -1, 1025):
        assert sn(100, fake, 16, n, 1234, 0, None, None, fake, None) == -1
        assert b"N must be in 1..1024" in lib.tlsan_last_error()
    assert sn(100, fake, 16, 10, 1234, 0, fake, None, fake, None) == -1     # the CSR comes as a pair
    assert sn(100, fake, 16, 10, 1234, 0, None, fake, fake, None) == -1
    assert b"go together" in lib.tlsan_last_error()


def test_splitmix64_is_the_standard_finaliser():
    # SplitMix64 seeded with 0: its first outputs (the state advances by the golden gamma before each mix)
    with np.errstate(over="ignore"):
        assert int(splitmix64(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF
        assert int(splitmix64(np.array([0x9e3779b97f4a7c15], np.uint64))[0]) == 0x6E789E6AA1B965F4


def test_reference_negatives_are_distinct_eligible_and_padded():
    rng = np.random.RandomState(5)
    for item_count, n in ((22048, 100), (5000, 1024), (300, 50)):
        for row in (0, 1, 4095, 123456789, -3):
            label = int(rng.randint(item_count))
            excl = set(rng.randint(0, item_count, 20).tolist())
            neg = reference_negatives(item_count, label, excl, n, 1234, row)
            assert neg.shape == (n,) and (neg >= 0).all() and (neg < item_count).all()
            assert len(set(neg.tolist())) == n
            assert label not in neg and not (set(neg.tolist()) & excl)
    # fewer eligible items than n: every eligible item, then -1
    neg = reference_negatives(40, 3, {5, 6}, 50, 1234, 7)
    found = neg[neg >= 0]
    assert (neg[len(found):] == -1).all() and len(found) == 37
    assert set(found.tolist()) == set(range(40)) - {3, 5, 6}
    # the row's stream depends on the seed and the row, not on anything else
    a = reference_negatives(22048, 0, set(), 20, 1234, 10)
    assert not np.array_equal(a, reference_negatives(22048, 0, set(), 20, 1235, 10))
    assert not np.array_equal(a, reference_negatives(22048, 0, set(), 20, 1234, 11))
    assert np.array_equal(a[:10], reference_negatives(22048, 0, set(), 10, 1234, 10))   # a prefix of the longer list


def test_sampled_metrics_hand_computed():
    from tlsan_amd.model import metrics_from_histogram, rank_histogram, sampled_metrics
    ranks = np.array([0, 1, 5, 100, 3])
    m = sampled_metrics(ranks, 100)
    assert m["HR@1"] == pytest.approx(1 / 5, abs=1e-15)
    assert m["HR@5"] == pytest.approx(3 / 5, abs=1e-15)
    assert m["HR@10"] == pytest.approx(4 / 5, abs=1e-15) and m["HR@20"] == m["HR@10"]
    assert m["NDCG@1"] == pytest.approx(1 / 5, abs=1e-15)
    assert m["NDCG@5"] == pytest.approx((1 + 1 / np.log2(3) + 1 / np.log2(5)) / 5, abs=1e-15)
    assert m["NDCG@10"] == pytest.approx((1 + 1 / np.log2(3) + 1 / np.log2(5) + 1 / np.log2(7)) / 5, abs=1e-15)
    assert m["MRR"] == pytest.approx((1 + 1 / 2 + 1 / 6 + 1 / 101 + 1 / 4) / 5, abs=1e-15)
    assert m["AUC_N"] == pytest.approx(np.mean([1 - r / 100 for r in ranks]), abs=1e-15)
    assert list(m) == ["HR@1", "HR@5", "HR@10", "HR@20", "NDCG@1", "NDCG@5", "NDCG@10", "NDCG@20", "MRR", "AUC_N"]
    # histograms of parts add up to the whole: the metrics do not depend on the split
    h = rank_histogram(ranks[:2], 100) + rank_histogram(ranks[2:], 100)
    assert metrics_from_histogram(h, 100) == m
    assert sampled_metrics([0, 1], 1, ks=(1,)) == {"HR@1": 0.5, "NDCG@1": 0.5, "MRR": 0.75, "AUC_N": 0.5}
    with pytest.raises(ValueError):
        rank_histogram([0, 101], 100)


def test_driver_sampled_flags():
    from tlsan_amd.train import parse, sampled_line
    a = parse(["--dataset", "x.npz"])
    assert a.eval_negatives == 0 and a.eval_neg_seed == 1234 and a.eval_neg_exclude == "history"   # off by default
    a = parse(["--dataset", "x.npz", "--eval_negatives", "100", "--eval_neg_seed", "7", "--eval_neg_exclude", "none"])
    assert a.eval_negatives == 100 and a.eval_neg_seed == 7 and a.eval_neg_exclude == "none"
    with pytest.raises(SystemExit):
        parse(["--eval_neg_exclude", "all"])
    line = sampled_line(100, {"HR@1": 0.25, "MRR": 0.5})
    assert line == "Sampled N=100: HR@1 = 0.2500 MRR = 0.5000"

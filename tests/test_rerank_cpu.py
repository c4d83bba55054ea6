"""Diversified lists without a GPU: the ABI's addition, the argument checks of tlsan_rerank (refused before any launch),
the driver's flags, and the reference (tests/rerank_ref.py) on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import rerank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_exports():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    assert re.search(r"\bint\s+tlsan_rerank\(", hdr)
    assert "tlsan_rerank" in L.EXPORTS and hasattr(L.load(), "tlsan_rerank")
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and L.load().tlsan_abi_version() == 15
    assert L.RERANK_MAX == 256 == L.TOPK_MAX


def test_arguments_are_refused_without_a_launch():
    from tlsan_amd import _lib as L
    lib = L.load()
    err = lambda: lib.tlsan_last_error()

    def call(B=3, N=32, d=64, K=10, theta=0.5, m=0, **ptr):
        # NULL device pointers throughout: a call that got past the checks would fault at once
        p = dict(pool_ids=None, pool_scores=None, vec=None, inv=None, cate=None, ids=None, scores=None)
        p.update(ptr)
        return lib.tlsan_rerank(p["pool_ids"], p["pool_scores"], p["vec"], p["inv"], p["cate"], B, N, d, K, theta, m,
                                p["ids"], p["scores"], None)

    for kw in (dict(K=0), dict(K=33), dict(K=-1), dict(N=257), dict(N=0), dict(theta=-0.1), dict(theta=1.5),
               dict(theta=float("nan")), dict(m=-1), dict(B=0)):
        assert call(**kw) == -1, kw
        assert b"tlsan_rerank" in err(), (kw, err())
    assert call(d=96) == -4 and b"tlsan_rerank" in err()
    assert call() == -1 and b"tlsan_rerank: NULL" in err()          # good numbers, NULL pointers
    fake = 0x1000                                                   # (never dereferenced: one pointer stays NULL)
    names = ("pool_ids", "pool_scores", "vec", "inv", "cate", "ids", "scores")
    for hole in names:
        assert call(**{n: fake for n in names if n != hole}) == -1, hole
        assert b"tlsan_rerank: NULL" in err(), (hole, err())


def test_driver_parses_the_flags():
    from tlsan_amd import train as T
    a = T.parse(["--dataset", "x.npz"])
    assert (a.recommend_diversity, a.recommend_per_category, a.recommend_pool) == (0.0, 0, 0)
    assert T.recommend_settings(a) == {}
    a = T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_diversity", "0.25", "--recommend_per_category", "2",
                 "--recommend_pool", "64"])
    assert (a.recommend_diversity, a.recommend_per_category, a.recommend_pool) == (0.25, 2, 64)
    assert T.recommend_settings(a) == dict(diversity=0.25, per_category=2, pool=64)
    a = T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_per_category", "1"])
    assert T.recommend_settings(a) == dict(diversity=0.0, per_category=1, pool=None)


def test_pool_arguments():
    from tlsan_amd.model import rerank_chunk, rerank_pool
    assert rerank_pool(10, 0.0, 0, None) is None                    # the plain top-k path
    assert rerank_pool(10, 0.5, 0, None) == 40 and rerank_pool(3, 0.0, 1, None) == 32
    assert rerank_pool(100, 0.5, 0, None) == 256 and rerank_pool(10, 0.5, 2, 77) == 77
    for k, theta, m, pool in ((10, 0.5, 0, 300), (10, 0.5, 0, 5), (10, 2.0, 0, None), (10, -0.1, 0, None),
                              (10, float("nan"), 0, None), (10, 0.0, -1, None), (10, 0.0, 0, 64), (0, 0.5, 0, None),
                              (300, 0.5, 0, None)):
        with pytest.raises(ValueError):
            rerank_pool(k, theta, m, pool)
    assert rerank_chunk(256, 256) == 1024 and rerank_chunk(256, 256, 2) == 512
    assert rerank_chunk(256, 256) * 256 * 256 * 4 <= 256 << 20


def _pool(N, d, seed, ncat=4):
    rng = np.random.RandomState(seed)
    ids = rng.permutation(10 * N)[:N].astype(np.int32)
    s = np.sort(rng.standard_normal(N).astype(np.float32))[::-1].copy()
    w = rng.standard_normal((N, d)).astype(np.float32)
    inv = (1.0 / np.sqrt((w.astype(np.float64) ** 2).sum(1))).astype(np.float32)
    return ids, s, w, inv, rng.randint(0, ncat, N).astype(np.int32)


def test_reference_identity_prefix():
    ids, s, w, inv, cate = _pool(20, 8, 0)
    assert ref.select(ids, s, w, inv, cate, 7, 0.0, 0) == list(range(7))
    s[4], ids[9] = np.nan, -1                                       # invalid entries are passed over
    assert ref.select(ids, s, w, inv, cate, 7, 0.0, 0) == [0, 1, 2, 3, 5, 6, 7]
    s[~np.isnan(s)] = 1.5                                           # all equal: r = 0, the order of the positions
    assert ref.relevance(ids, s).tolist() == [0.0] * 20
    assert ref.select(ids, s, w, inv, cate, 20, 0.0, 0) == [j for j in range(20) if j not in (4, 9)]
    assert ref.select(np.full(3, -1), s[:3], w[:3], inv[:3], cate[:3], 2, 0.5, 0) == []


def test_reference_cap_is_honoured():
    ids, s, w, inv, cate = _pool(40, 8, 1, ncat=5)
    for theta in (0.0, 0.6):
        for m in (1, 2, 3):
            picks = ref.select(ids, s, w, inv, cate, 40, theta, m)
            assert np.bincount(cate[picks], minlength=5).max() <= m
            assert len(picks) == sum(min(m, int((cate == c).sum())) for c in range(5))     # and the list ends short
            regret, was, more = ref.replay(ids, s, w, inv, cate, theta, m, picks)
            assert was.all() and not more and np.all(regret == 0)
    picks = ref.select(ids, s, w, inv, cate, 40, 0.0, 1)
    bad = picks[:2] + [int(np.flatnonzero(cate == cate[picks[0]])[1])]      # a second item of the first pick's category
    assert not ref.replay(ids, s, w, inv, cate, 0.0, 1, bad)[1][2]


def test_reference_duplicates_tie_to_the_lower_position():
    ids, s, w, inv, cate = _pool(6, 8, 2)
    s[:] = 0.25                                                     # relevance out of the way
    w[4], inv[4] = w[2], inv[2]
    picks = ref.select(ids, s, w, inv, cate, 6, 0.5, 0)
    assert picks[0] == 0 and picks.index(2) < picks.index(4)
    assert picks[-1] == 4                                           # cos = 1 against its twin: the last one wanted
    regret, was, more = ref.replay(ids, s, w, inv, cate, 0.5, 0, picks)
    assert was.all() and not more and np.all(regret == 0)
    swapped = [4 if j == 2 else 2 if j == 4 else j for j in picks]
    assert np.all(ref.replay(ids, s, w, inv, cate, 0.5, 0, swapped)[0] == 0)     # the same values: only the tie rule differs
    w[3] = 0.0
    inv[3] = 0.0                                                    # a zero row: cos 0 against everything
    row = ref._Row(ids, s, w, inv, cate, 0.5, 0)
    row.take(0)
    assert row.maxcos[3] == 0.0


def test_reference_penalty_moves_a_near_duplicate_down():
    w = np.array([[1, 0], [1, 0.01], [0, 1]], np.float32)
    inv = (1.0 / np.sqrt((w.astype(np.float64) ** 2).sum(1))).astype(np.float32)
    ids, s, cate = np.arange(3, dtype=np.int32), np.array([3, 2, 1], np.float32), np.zeros(3, np.int32)
    assert ref.select(ids, s, w, inv, cate, 3, 0.0, 0) == [0, 1, 2]
    assert ref.select(ids, s, w, inv, cate, 3, 0.5, 0) == [0, 2, 1]
    regret, was, _ = ref.replay(ids, s, w, inv, cate, 0.5, 0, [0, 1, 2])
    assert was.all() and regret[1] > 0.2 and regret[0] == 0 == regret[2]


def test_reference_capped_list_over_a_full_pool_is_the_brute_force_ranking():
    rng = np.random.RandomState(3)
    I, d = 120, 8
    s = rng.standard_normal(I).astype(np.float32)
    s[rng.randint(0, I, 30)] = s[rng.randint(0, I, 30)]            # ties between ids
    cate = rng.randint(0, 9, I).astype(np.int32)
    order = np.lexsort((np.arange(I), -s.astype(np.float64)))       # tlsan_eval_topk's order: the pool holds every item
    w = rng.standard_normal((I, d)).astype(np.float32)
    inv = np.ones(I, np.float32)
    for K, m in ((10, 1), (10, 2), (40, 3)):
        picks = ref.select(order.astype(np.int32), s[order], w[order], inv[order], cate[order], K, 0.0, m)
        assert order[picks].tolist() == ref.capped_ranking(s, cate, K, m)
    assert ref.positions(np.array([7, 5, 9, -1]), np.array([9, 7, -1])) == [2, 0]
    with pytest.raises(AssertionError):
        ref.positions(np.array([7, 5, 9]), np.array([9, 4, -1]))

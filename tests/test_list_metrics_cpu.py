"""List metrics without a GPU: the ABI's addition, the argument checks of tlsan_list_metrics (refused before any launch),
the Python checks, the driver's flag, the reference (tests/list_metrics_ref.py) and the counters on hand-made rows, and
input.item_self_information on a training set worked by hand."""
import math
import os
import re

import numpy as np
import pytest

from tests import list_metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ILD@%d", "categories@%d", "max_per_category", "HR@%d", "NDCG@%d", "MRR@%d", "novelty@%d", "coverage@%d", "gini@%d",
        "rows", "short_rows")


def test_header_and_exports():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    assert re.search(r"\bint\s+tlsan_list_metrics\(", hdr)
    assert "tlsan_list_metrics" in L.EXPORTS and hasattr(L.load(), "tlsan_list_metrics")
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and L.load().tlsan_abi_version() == 15
    assert L.LISTM_MAX == 256 == L.TOPK_MAX == L.RERANK_MAX
    from tlsan_amd import build
    assert "tlsan_listm.hip" in build.SOURCES


def test_arguments_are_refused_without_a_launch():
    from tlsan_amd import _lib as L
    lib = L.load()
    err = lambda: lib.tlsan_last_error()
    needed = ("ids", "vec", "inv", "cate", "n_valid", "pair_cos", "n_cate", "max_cate", "hit_pos", "weight_sum")
    fake = 0x1000                                                   # (never dereferenced: every call below is refused)

    def call(B=3, K=10, d=64, n_items=0, **ptr):
        p = dict.fromkeys(needed + ("labels", "weight", "exposure"))
        p.update(ptr)
        return lib.tlsan_list_metrics(p["ids"], p["vec"], p["inv"], p["cate"], p["labels"], p["weight"], B, K, d,
                                      p["n_valid"], p["pair_cos"], p["n_cate"], p["max_cate"], p["hit_pos"], p["weight_sum"],
                                      p["exposure"], n_items, None)

    full = {n: fake for n in needed}
    for kw in (dict(B=0), dict(B=-2), dict(K=0), dict(K=257), dict(K=-1), dict(exposure=fake, n_items=0),
               dict(exposure=fake, n_items=-5), dict(B=1 << 24, K=256)):
        assert call(**dict(full, **kw)) == -1, kw                   # TLSAN_E_BADARG, with every pointer given
        assert b"tlsan_list_metrics" in err(), (kw, err())
    assert call(**dict(full, d=96)) == -4 and b"tlsan_list_metrics" in err()      # TLSAN_E_UNSUPPORTED
    assert call() == -1 and b"tlsan_list_metrics: NULL" in err()    # good numbers, NULL pointers
    for hole in needed:
        assert call(**{n: fake for n in needed if n != hole}) == -1, hole
        assert b"tlsan_list_metrics: NULL" in err(), (hole, err())
    # (labels, weight and exposure may be NULL: with the ten others given such a call would launch, so it is not made here)


def test_python_arguments():
    import torch
    from tlsan_amd.model import list_metric_inputs
    ok = np.zeros((3, 10), np.int32)
    ids, labels, w = list_metric_inputs(ok, [1, 2, 3], np.ones(50, np.float32), None, 50, "cpu")
    assert ids.dtype == torch.int32 and labels.dtype == torch.int32 and w.dtype == torch.float32
    assert list_metric_inputs(torch.zeros(2, 256, dtype=torch.int64), None, None, None, 50, "cpu")[1:] == (None, None)
    for bad in (np.zeros(10, np.int32), np.zeros((2, 3, 4), np.int32), np.zeros((3, 0), np.int32), np.zeros((3, 257), np.int32),
                np.zeros((0, 5), np.int32), np.full((3, 10), 50, np.int32)):
        with pytest.raises(ValueError):
            list_metric_inputs(bad, None, None, None, 50, "cpu")
    for kw in (dict(labels=[1, 2]), dict(labels=np.zeros((3, 1))), dict(item_weight=np.ones(49)), dict(item_weight=np.ones((50, 1))),
               dict(exposure=np.zeros(50, np.int32)), dict(exposure=torch.zeros(50, dtype=torch.int64)),
               dict(exposure=torch.zeros(49, dtype=torch.int32))):
        args = dict(labels=None, item_weight=None, exposure=None)
        args.update(kw)
        with pytest.raises(ValueError):
            list_metric_inputs(ok, args["labels"], args["item_weight"], args["exposure"], 50, "cpu")


def test_driver_parses_the_flag():
    from tlsan_amd import train as T
    assert T.parse(["--dataset", "x.npz"]).recommend_metrics == 0
    assert T.parse(["--dataset", "x.npz", "--recommend_k", "5"]).recommend_metrics == 0
    assert T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_metrics", "1"]).recommend_metrics == 1
    with pytest.raises(SystemExit):
        T.parse(["--dataset", "x.npz", "--recommend_metrics", "1"])
    assert T.list_metrics_path("m", 5) == os.path.join("m", "recommend_top5_metrics.json")


def _unit(*rows_):
    w = np.array(rows_, np.float32)
    ss = (w.astype(np.float64) ** 2).sum(1)
    return w, np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32)


def test_reference_pairs():
    w, inv = _unit([3, 4], [3, 4])
    r = ref.row([7, 8], w, inv, [0, 0])
    assert r["n"] == 2 and abs(r["ild"]) < 1e-6 and abs(r["pair_cos"] - 1.0) < 1e-6        # two identical vectors
    w, inv = _unit([2, 0, 0], [0, 5, 0], [0, 0, 1])
    r = ref.row([1, 2, 3], w, inv, [0, 1, 2])
    assert r["ild"] == 1.0 and r["pair_cos"] == 0.0                                         # orthogonal vectors
    w, inv = _unit([1, 0], [0, 0], [1, 0])
    r = ref.row([1, 2, 3], w, inv, [0, 0, 0])
    assert inv[1] == 0.0 and abs(r["pair_cos"] - 1.0) < 1e-6 and abs(r["ild"] - (1.0 - 1.0 / 3.0)) < 1e-6   # a zero vector: cos 0
    for ids in ([5], [-1, 5, -1], [-1, -1], []):                                            # n < 2
        k = len(ids)
        r = ref.row(ids, np.ones((k, 2), np.float32), np.ones(k, np.float32), [0] * k)
        assert r["n"] == sum(i >= 0 for i in ids) and math.isnan(r["ild"]) and r["pair_cos"] == 0.0
    # holes are skipped: the entry in the hole is not looked at, whatever it holds
    w, inv = _unit([1, 0], [9, 9], [0, 1], [1, 1])
    a = ref.row([4, -1, 6, 2], w, inv, [0, 5, 1, 1])
    b = ref.row([4, 6, 2], w[[0, 2, 3]], inv[[0, 2, 3]], [0, 1, 1])
    assert a["n"] == 3 and a["pair_cos"] == b["pair_cos"] and a["ild"] == b["ild"] and a["n_cate"] == b["n_cate"] == 2


def test_reference_categories_and_hits():
    w, inv = _unit(*[[1.0, j] for j in range(5)])
    r = ref.row([10, 11, 12, -1, 13], w, inv, [3, 3, 5, 3, 3])                              # categories [3, 3, 5, -, 3]
    assert (r["n"], r["n_cate"], r["max_cate"]) == (4, 2, 3)
    assert ref.row([-1, -1], w[:2], inv[:2], [1, 1])["max_cate"] == 0
    ids = [4, -1, 9, 9, 2]
    assert ref.row(ids, w, inv, [0] * 5, label=9)["hit_pos"] == 2                            # the first of two duplicates; holes count
    assert ref.row(ids, w, inv, [0] * 5, label=2)["hit_pos"] == 4
    assert ref.row(ids, w, inv, [0] * 5, label=3)["hit_pos"] == -1                           # absent
    assert ref.row(ids, w, inv, [0] * 5, label=-1)["hit_pos"] == -1                          # negative: never the hole
    assert ref.row(ids, w, inv, [0] * 5)["hit_pos"] == -1
    r = ref.row(ids, w, inv, [0] * 5, weight=[1.5, 100.0, 2.0, 2.0, 0.25])
    assert r["weight_sum"] == 5.75


def test_gini_and_coverage():
    from tlsan_amd.model import exposure_stats
    I = 7
    assert ref.gini(np.full(I, 3)) == 0.0 and exposure_stats(np.full(I, 3, np.int32), I) == (1.0, 0.0)
    one = np.zeros(I, np.int32)
    one[4] = 11
    assert abs(ref.gini(one) - (I - 1) / I) < 1e-15
    cov, g = exposure_stats(one, I)
    assert cov == 1.0 / I and abs(g - (I - 1) / I) < 1e-15
    x = np.array([0, 5, 1, 0, 9, 2, 2], np.int32)
    cov, g = exposure_stats(x, I)
    assert cov == 5.0 / I and abs(g - ref.gini(x)) < 1e-15
    cov, g = exposure_stats(np.zeros(I, np.int32), I)
    assert cov == 0.0 and math.isnan(g)
    assert exposure_stats(np.array([-1, 1], np.int32), 2)[1] > 0.49                          # int32 counters are read as uint32


def _made_up(B=23, K=6, d=4, I=30, seed=5):
    rng = np.random.RandomState(seed)
    ids = rng.randint(-1, I, (B, K)).astype(np.int32)
    ids[3], ids[4, 1:] = -1, -1
    w = rng.standard_normal((B, K, d)).astype(np.float32)
    inv = (1.0 / np.sqrt((w.astype(np.float64) ** 2).sum(2))).astype(np.float32)
    cate = rng.randint(0, 4, (B, K)).astype(np.int32)
    labels = np.where(rng.rand(B) < 0.6, ids[:, 2], rng.randint(-1, I, B)).astype(np.int32)
    weight = rng.rand(B, K).astype(np.float32) * 8
    return ids, ref.rows(ids, w, inv, cate, labels, weight), ref.exposure(ids, I), I, K


def _as_metrics(m):
    import torch
    from tlsan_amd.model import ListMetrics
    t = lambda k, dt: torch.as_tensor(np.ascontiguousarray(m[k])).to(dt)
    return ListMetrics(t("n", torch.int32), t("pair_cos", torch.float64), t("ild", torch.float64), t("n_cate", torch.int32),
                       t("max_cate", torch.int32), t("hit_pos", torch.int32), t("weight_sum", torch.float64))


def _same(a, b, rel=1e-12):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], int) or isinstance(b[k], int):
            assert a[k] == b[k], k
        else:
            assert (math.isnan(a[k]) and math.isnan(b[k])) or abs(a[k] - b[k]) <= rel * abs(b[k]), (k, a[k], b[k])


def test_counters_do_not_depend_on_the_split():
    from tlsan_amd.model import ListMetricCounters
    ids, m, expo, I, K = _made_up()
    want = ref.result(m, K, expo)
    assert list(want) == [k % K if "%" in k else k for k in KEYS]
    assert want["rows"] == 23 and want["short_rows"] >= 2 and 0 < want["HR@6"] < 1 and want["NDCG@6"] <= want["HR@6"]
    cuts = [(0, 23)], [(0, 5), (5, 6), (6, 23)], [(0, 0), (0, 23)]
    for cut in cuts:
        c = ListMetricCounters()
        for lo, hi in cut:
            c.add(_as_metrics(ref.take(m, slice(lo, hi))), K)
        _same(c.result(expo.astype(np.int32), I), want)
        _same(ref.result({k: np.concatenate([v[lo:hi] for lo, hi in cut]) for k, v in m.items()}, K, expo), want)
    none = c.result()
    assert math.isnan(none["coverage@6"]) and math.isnan(none["gini@6"]) and none["rows"] == 23
    # two processes' counters add up (reduce): both hold half, the total is formed by the callback
    halves = []
    for lo, hi in ((0, 11), (11, 23)):
        c = ListMetricCounters()
        c.add(_as_metrics(ref.take(m, slice(lo, hi))), K)
        halves.append(c)
    for name in ("_int", "_dbl"):
        total = getattr(halves[0], name) + getattr(halves[1], name)
        setattr(halves[0], name, total)
    halves[0].reduce(lambda t: t)
    _same(halves[0].result(expo, I), want)
    with pytest.raises(ValueError):
        c.add(_as_metrics(m), K + 1)
    with pytest.raises(ValueError):
        ListMetricCounters().result()


def test_item_self_information_by_hand():
    from tlsan_amd.input import PackedSet, item_self_information
    # five samples: positives 2, 2, 0 (label 1); targets 3, 1 are sampled negatives (label 0)
    samples = [(0, [1], [2], [0.0], 2, 1, 0), (1, [], [1], [], 3, 0, 0), (0, [1, 2], [0], [0.0, 1.0], 2, 1, 0),
               (2, [3], [3], [0.0], 0, 1, 1), (1, [0], [2], [0.0], 1, 0, 1)]
    got = item_self_information(PackedSet.from_samples(samples), 4)
    want = -np.log2(np.array([2.0, 1.0, 3.0, 1.0]) / 9.0)           # (c + 1) / (T + I), T = 5, I = 4
    assert got.dtype == np.float32 and got.shape == (4,) and np.array_equal(got, want.astype(np.float32))
    assert got[1] == got[3] > got[0] > got[2] > 0
    with pytest.raises(ValueError):
        item_self_information(PackedSet.from_samples(samples), 2)   # a positive outside the table

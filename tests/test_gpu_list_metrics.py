"""GPU tests of the list metrics (tlsan_list_metrics, Model.list_metrics, the driver's --recommend_metrics) against the
fp64 reference of tests/list_metrics_ref.py.  Integer outputs and the exposure counter are compared for equality, ILD
within rerank_ref.tau(d) = 8 d 2^-24 (derived in list_metrics_ref's header, not measured), weight_sum within 1e-12
relative; pair_cos of the same list has the same bits in any batch and on a second run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import list_metrics_ref as ref
from tests.helpers import batch_tuple, host, make_config, random_batch, random_params
from tests.rerank_ref import tau

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 37
SPECIAL = tuple(range(3, 15))
CASES = [(64, 1), (64, 2), (64, 17), (128, 64), (128, 65), (128, 100), (256, 256)]
NAMES = ("n", "pair_cos", "ild", "n_cate", "max_cate", "hit_pos", "weight_sum")


def make_lists(d, K, seed, rows=B, n_items=None):
    """Made-up lists [rows, K] as tests/test_gpu_rerank.make_pools builds its pools -- distinct ids, vectors around 8
    cluster centres, categories from 12 values, inv = 1 / |w| rounded to fp32 -- with labels, weights and the special
    rows 3 .. 14 (each as far as K allows)."""
    rng = np.random.RandomState(seed)
    I = n_items or 10 * K + 7
    centres = rng.standard_normal((8, d))
    ids = np.stack([rng.permutation(I)[:K] for _ in range(rows)]).astype(np.int32)
    w = (centres[rng.randint(0, 8, (rows, K))] + 0.35 * rng.standard_normal((rows, K, d))).astype(np.float32)
    cate = rng.randint(0, 12, (rows, K)).astype(np.int32)
    weight = (rng.rand(rows, K) * 12).astype(np.float32)
    labels = np.where(rng.rand(rows) < 0.5, ids[np.arange(rows), rng.randint(0, K, rows)], I + 5).astype(np.int32)
    last = K - 1
    ids[3] = -1                                                      # all -1
    ids[4], ids[4, K // 2] = -1, 11                                  # exactly one valid entry
    ids[5, 1:last:3] = -1                                            # holes in the middle
    ids[6, K - max(1, K // 4):] = -1                                 # a -1 tail
    if K > 3:
        w[7, 3] = w[7, 1]                                            # two identical vectors
        ids[9, 3] = ids[9, 1]                                        # a repeated id ...
        ids[14, 3] = ids[14, 1]
    w[8, K // 2] = 0.0                                               # a zero vector with inv 0
    labels[9] = ids[9, min(1, last)]                                 # ... that is the label: its first position counts
    labels[10] = ids[10, 0]                                          # the label at position 0
    ids[11, last] = -1 if K > 1 else ids[11, last]
    labels[11] = ids[11, max(0, last - 1)]                           # the label at the last valid position
    labels[12] = I + 1                                               # the label absent
    labels[13] = -1                                                  # the label -1, in a row with holes
    ids[13, ::2] = -1
    w[ids < 0] = 0.0                                                 # tlsan_item_vectors writes zeros for -1
    ss = (w.astype(np.float64) ** 2).sum(2)
    inv = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32)
    return dict(ids=ids, w=w, inv=inv, cate=cate, labels=labels, weight=weight), I


def run(lists, n_items, rows=None, plain=False, exposure=None):
    """tlsan_list_metrics on the lists (rows: a subset, as a batch of its own; plain: labels, weight and exposure NULL)
    -> (dict of host arrays, exposure counter as int64 host array or None)."""
    import torch
    from tlsan_amd import _lib as L
    from tlsan_amd import model as M
    sel = slice(None) if rows is None else list(rows)
    dev = "cuda:0"
    t = {k: torch.as_tensor(np.ascontiguousarray(v[sel])).to(dev) for k, v in lists.items()}
    n, K = t["ids"].shape
    if exposure is None and not plain:
        exposure = torch.zeros(n_items, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    m = M.list_metrics(L.load(), t["ids"], t["w"].view(n * K, -1), t["inv"].view(-1), t["cate"].view(-1),
                       None if plain else t["labels"], None if plain else t["weight"].view(-1),
                       None if plain else exposure, st)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in zip(NAMES, m)}, exposure


def same_bits(a, b):
    for k in NAMES:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int64 if x.dtype == np.float64 else x.dtype),
                                                     y.view(np.int64 if y.dtype == np.float64 else y.dtype)), k


@pytest.mark.parametrize("d,K", CASES)
def test_kernel_against_the_reference(d, K):
    lists, I = make_lists(d, K, seed=3000 + d + K)
    got, expo = run(lists, I)
    want = ref.rows(*[lists[k] for k in ("ids", "w", "inv", "cate", "labels", "weight")])
    assert got["n"].dtype == np.int32 and got["pair_cos"].dtype == np.float64 and got["n"].shape == (B,)
    for k in ("n", "n_cate", "max_cate", "hit_pos"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    two = want["n"] >= 2
    err = np.abs(got["ild"][two] - want["ild"][two])
    print("d %d K %d: largest ILD error %.3g of tau %.3g over %d rows" % (d, K, err.max() if two.any() else 0.0, tau(d), two.sum()))
    assert np.all(err <= tau(d))
    assert np.all(np.isnan(got["ild"][~two])) and np.all(got["pair_cos"][~two] == 0.0) and not np.signbit(got["pair_cos"][~two]).any()
    assert np.all(np.abs(got["weight_sum"] - want["weight_sum"]) <= 1e-12 * np.abs(want["weight_sum"]))
    assert got["n"][3] == 0 and got["max_cate"][3] == 0 and got["n"][4] == 1 and got["hit_pos"][12] == -1 == got["hit_pos"][13]
    if K > 3:
        assert got["hit_pos"][9] == 1 and got["hit_pos"][10] == 0 and got["hit_pos"][11] == K - 2
    # the exposure counter: one call, and exactly twice that after a second call on the same counter
    count = ref.exposure(lists["ids"], I)
    assert np.array_equal(host(expo).astype(np.int64), count)
    again, expo = run(lists, I, exposure=expo)
    assert np.array_equal(host(expo).astype(np.int64), 2 * count)
    # bits: the same call again; the special rows as a batch of their own; without labels, weight and exposure
    same_bits(got, again)
    alone, _ = run(lists, I, rows=SPECIAL)
    same_bits(alone, ref.take(got, list(SPECIAL)))
    bare, none = run(lists, I, plain=True)
    assert none is None and np.all(bare["hit_pos"] == -1) and np.all(bare["weight_sum"] == 0.0)
    same_bits({k: bare[k] for k in NAMES if k not in ("hit_pos", "weight_sum")} | {k: got[k] for k in ("hit_pos", "weight_sum")}, got)


def test_ids_past_the_counter_are_skipped():
    lists, I = make_lists(64, 17, seed=77)
    import torch
    expo = torch.zeros(40, dtype=torch.int32, device="cuda:0")      # a counter over the first 40 items only
    got, expo = run(lists, 40, exposure=expo)
    assert np.array_equal(host(expo).astype(np.int64), ref.exposure(lists["ids"], 40))
    assert np.array_equal(got["n"], (lists["ids"] >= 0).sum(1))


# ---- through Model
def _stored(m, cat):
    """w_g = [item_emb[g] || cate_emb[item_cate[g]]] from get_params (the stored, rounded tables) and 1 / |w_g| in fp64"""
    p = m.get_params()
    w = np.concatenate([p["item_emb"], p["cate_emb"][np.asarray(cat)]], 1).astype(np.float64)
    ss = (w ** 2).sum(1)
    return w, np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)


def _reference(m, cat, ids, labels=None, item_weight=None):
    w, inv = _stored(m, cat)
    g = np.maximum(ids, 0)
    return ref.rows(ids, w[g], inv[g], np.asarray(cat)[g], labels, None if item_weight is None else item_weight[g])


@pytest.fixture(scope="module", params=["f32", "bf16"])
def model_case(request):
    from tlsan_amd.model import Model
    cfg = make_config(U=40, I=200, C=7, d=64)
    p = random_params(cfg, seed=71)
    b, cat = random_batch(cfg, B=29, Sn=3, seed=72, test=True)
    m = Model(cfg, cat, table_dtype=request.param)
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    return m, b, cat


def test_model_list_metrics_of_diversified_lists(model_case):
    import torch
    m, b, cat = model_case
    ids = m.recommend(batch_tuple(b, True), 10, exclude="history", diversity=0.5)[0]
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.cate_emb, m.item_b, m.dense)]
    before = snap()
    weight = np.random.RandomState(5).rand(200).astype(np.float32) * 9
    expo = torch.zeros(200, dtype=torch.int32, device=m.device)
    got = m.list_metrics(ids, labels=b["i"], item_weight=weight, exposure=expo)
    after = snap()
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, after))
    got = {k: host(v) for k, v in zip(NAMES, got)}
    want = _reference(m, cat, host(ids), b["i"], weight)
    for k in ("n", "n_cate", "max_cate", "hit_pos"):
        assert np.array_equal(got[k], want[k]), k
    assert np.all(want["n"] == 10) and np.all(np.abs(got["ild"] - want["ild"]) <= tau(64))
    assert np.all(np.abs(got["weight_sum"] - want["weight_sum"]) <= 1e-12 * want["weight_sum"])
    assert np.array_equal(host(expo).astype(np.int64), ref.exposure(host(ids), 200))
    # an array of ids and the tensor give the same bits; wrong arguments are refused
    same_bits(got, {k: host(v) for k, v in zip(NAMES, m.list_metrics(host(ids), labels=b["i"], item_weight=weight))})
    for bad in (dict(ids=host(ids)[0]), dict(ids=np.zeros((2, 257), np.int32)), dict(ids=np.full((2, 3), 200)),
                dict(ids=host(ids), labels=b["i"][:5]), dict(ids=host(ids), item_weight=weight[:100])):
        with pytest.raises(ValueError):
            m.list_metrics(**bad)


def test_model_cap_and_hits(model_case):
    m, b, cat = model_case
    capped = m.recommend(batch_tuple(b, True), 10, per_category=2, pool=256)[0]
    mc = host(m.list_metrics(capped).max_cate)
    assert np.all(mc <= 2) and (mc == 2).any()
    plain = m.recommend(batch_tuple(b, True), 10)[0]
    hit = host(m.list_metrics(plain, labels=b["i"]).hit_pos)
    found = (host(plain) == np.asarray(b["i"])[:, None]).any(1)
    assert np.array_equal(hit >= 0, found)
    assert np.array_equal(hit[found], (host(plain) == np.asarray(b["i"])[:, None]).argmax(1)[found])


# ---- the driver
def test_driver_measures_its_lists(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    base = [sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--max_steps", "3", "--eval_freq", "1000", "--quiet",
            "--recommend_k", "5", "--recommend_per_category", "1"]
    out = str(tmp_path / "model")
    r = subprocess.run(base + ["--model_dir", out, "--recommend_metrics", "1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.load(open(os.path.join(out, "recommend_top5_metrics.json")))
    for k in ("ILD@5", "categories@5", "max_per_category", "HR@5", "NDCG@5", "MRR@5", "novelty@5", "coverage@5", "gini@5",
              "rows", "short_rows"):
        assert k in res, k
    assert res["max_per_category"] == 1 and 0 < res["coverage@5"] <= 1 and 0 <= res["gini@5"] < 1
    assert res["rows"] == len(np.load(ds)["test_u"]) and (res["diversity"], res["per_category"], res["pool"]) == (0.0, 1, 0)
    assert 0 <= res["NDCG@5"] <= res["HR@5"] <= 1 and res["novelty@5"] > 0 and res["categories@5"] <= 5
    # the lists' file keeps the keys it has without the flag (what test_gpu_rerank's driver test reads, and no other)
    z = np.load(os.path.join(out, "recommend_top5.npz"))
    assert sorted(z.files) == ["diversity", "ids", "per_category", "pool", "scores", "user"]
    # the file's numbers are those of the lists it sits beside
    ids = z["ids"]
    assert ids.shape == (res["rows"], 5)
    assert res["short_rows"] == int(((ids >= 0).sum(1) < 5).sum())
    assert abs(res["coverage@5"] - len(np.unique(ids[ids >= 0])) / len(np.load(ds)["item_cate_list"])) < 1e-12

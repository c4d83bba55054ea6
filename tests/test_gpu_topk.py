"""GPU tests of the top-K recommendation over all items (tlsan_eval_topk / tlsan_topk_merge, Model.recommend,
ShardedModel.recommend, the driver's --recommend_k): against the fp64 oracle, bit for bit against the rank path, and
the order's corner cases (exact ties, NaN, exclusion, rows with fewer than K eligible items)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.helpers import (batch_tuple, history_sets, host, label_scores, make_config, model, p32, random_batch,
                           random_params)
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_order(ids, scores):
    """scores non-increasing along a row, equal scores with ascending ids, valid entries before the padding"""
    s = scores.astype(np.float64)
    valid = ids >= 0
    assert np.all(valid[:, :-1] | ~valid[:, 1:])
    both = valid[:, :-1] & valid[:, 1:]
    a, b = s[:, :-1], s[:, 1:]
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    ok = np.where(nan_a, nan_b, nan_b | (a > b) | ((a == b) & (ids[:, :-1] < ids[:, 1:])))
    assert np.all(ok | ~both)
    assert np.all(scores[~valid] == -np.inf)


def _oracle_topk(scores, k):
    """ids of the oracle's top k and the rows on which they are unambiguous at fp32 resolution"""
    ids = orc.topk_ids(scores, k + 1)
    s = np.take_along_axis(scores, ids, 1)
    clear = (s[:, :k] - s[:, 1:k + 1]).min(1) > 1e-4
    return ids[:, :k], s[:, :k], clear


@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (64, 4), (128, 16), (128, 4)])
def test_topk_matches_oracle(d, H):
    cfg = make_config(U=60, I=700, C=13, d=d, H=H)
    p = p32(random_params(cfg, seed=51))
    b, cat = random_batch(cfg, B=77, Sn=3, seed=52, test=True)
    m = model(cfg, cat, p)
    ref = orc.forward(p, cat, b, H)
    scores = orc.all_item_scores(p, cat, ref["u_t"])
    for k in (1, 20, 100):
        ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), k))
        want, ws, clear = _oracle_topk(scores, k)
        assert ids.shape == (77, k) and sc.dtype == np.float32
        assert clear.sum() > (60 if k < 100 else 15), clear.sum()
        assert np.array_equal(ids[clear], want[clear])
        got_s = np.take_along_axis(scores, ids.astype(np.int64), 1)
        assert np.abs(sc - got_s).max() < 1e-4          # the returned score is the returned item's
        assert np.abs(sc - ws).max() < 1e-4
        _check_order(ids, sc)


@pytest.mark.parametrize("form,table_dtype", [("dense", "f32"), ("dense", "bf16"), ("gather", "f32"), ("gather", "bf16")])
def test_topk_consistent_with_label_ranks(form, table_dtype):
    """Lazy L2 (P != 1 after two steps): the label sits at position label_ranks[b] of its row with the score
    tlsan_eval_label_scores gives it, bit for bit, or is absent when its rank is >= K."""
    I = 2000 if form == "dense" else 270000          # gather: I * d * 4 B > 256 MB
    cfg = make_config(U=300, I=I, C=31, d=256)
    p = random_params(cfg, seed=61)
    tb, cat = random_batch(cfg, B=256, Sn=3, seed=62)
    b, _ = random_batch(cfg, B=512, Sn=3, seed=63, test=True)
    m = model(cfg, cat, p, l2_mode="lazy", table_dtype=table_dtype)
    for _ in range(2):
        m.train(None, (tb["u"], tb["i"], tb["y"], tb["hist_i"], tb["hist_i_new"], tb["hist_t"], tb["sl"], tb["sl_new"],
                       tb["u_cate"]), 1.0)
    assert m.table_scale() != 1.0
    K = 50
    # labels: every other row takes an item of its own list (u_t does not depend on the label), the rest stay random
    first = host(m.recommend(batch_tuple(b, True), K)[0])
    b["i"][::2] = first[np.arange(0, 512, 2), np.arange(256) % K]
    b["i"][::6] = first[::6, K - 1]
    ranks = host(m.label_ranks(batch_tuple(b, True)))
    _, _, ut, db = m.forward(batch_tuple(b, True), is_test=True, want_u_t=True)
    slab = label_scores(m, db, ut)
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), K))
    _check_order(ids, sc)
    assert (ranks < K).sum() >= 256
    pos = np.array([list(r).index(l) if l in r else K for r, l in zip(ids, b["i"])])
    hit = pos < K
    assert np.array_equal(sc[hit, pos[hit]].view(np.int32), slab[hit].view(np.int32))
    if form == "gather":
        assert np.array_equal(pos, np.minimum(ranks, K))
    else:
        # k_eval_rank_dense contracts (acc * P) + bias into one FMA (the label's own score is two roundings): its count
        # may differ from the selection's where an item's score lies within an ulp or two of the label's
        bad = pos != np.minimum(ranks, K)
        assert bad.sum() <= 2, bad.sum()
        for r in np.nonzero(bad)[0]:
            assert np.abs(sc[r].astype(np.float64) - slab[r]).min() <= 4 * np.spacing(np.float32(slab[r]))


def test_topk_exact_ties():
    cfg = make_config(U=20, I=300, C=5, d=64)
    p = p32(random_params(cfg, seed=71))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=72, test=True)
    tied = np.arange(100, 300, 5)[:40]             # 40 items, bit-identical rows, far ahead of the rest
    p["item_emb"][tied] = p["item_emb"][tied[0]]
    p["item_b"][tied] = 1000.0
    cat[tied] = cat[tied[0]]
    m = model(cfg, cat, p)
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 10))
    assert np.all(ids == tied[:10][None, :])
    assert np.all(sc == sc[:, :1])
    # a tie straddling the K boundary: 5 distinct leaders, then the tied group -> its 5 lowest ids
    lead = np.array([3, 17, 41, 77, 99])
    p["item_b"][lead] = 2000.0 + 100.0 * np.arange(5)
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 10))
    assert np.all(ids[:, :5] == lead[::-1][None, :])
    assert np.all(ids[:, 5:] == tied[:5][None, :])
    _check_order(ids, sc)


def test_topk_deterministic_and_batch_independent():
    cfg = make_config(U=300, I=9000, C=40, d=128)
    p = p32(random_params(cfg, seed=81))
    b, cat = random_batch(cfg, B=4096, Sn=3, seed=82, test=True)
    m = model(cfg, cat, p)
    from tlsan_amd.model import eval_topk, exclusion_csr
    _, _, ut, db = m.forward(batch_tuple(b, True), is_test=True, want_u_t=True)
    sub = {key: v[100:116] for key, v in b.items()}
    _, _, ut_s, db_s = m.forward(batch_tuple(sub, True), is_test=True, want_u_t=True)
    ut_s.copy_(ut[100:116])     # (the forward's own last bits may follow the launch's batch; the selection's may not)
    for k in (10, 256):
        a = [host(t) for t in m.recommend(batch_tuple(b, True), k)]
        a2 = [host(t) for t in m.recommend(batch_tuple(b, True), k)]
        assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1].view(np.int32), a2[1].view(np.int32))
        _check_order(*a)
        # a batch of 16 (36 item slices) and one of 4096 (8 slices), the same u_t rows
        run = lambda u, d: [host(t) for t in eval_topk(m.lib, m.dims, m.cparams, u, d.B, k, exclusion_csr(d, "history", 9000),
                                                        1, 0, m._topk_workspace, m._stream())]
        s, full = run(ut_s, db_s), run(ut, db)
        assert np.array_equal(s[0], full[0][100:116]) and np.array_equal(s[1].view(np.int32), full[1][100:116].view(np.int32))
        # end to end (each batch through its own forward): the same items
        e2e = host(m.recommend(batch_tuple(sub, True), k, exclude="history")[0])
        assert np.array_equal(e2e, full[0][100:116])


def test_topk_exclusion():
    cfg = make_config(U=60, I=800, C=13, d=128)
    p = p32(random_params(cfg, seed=91))
    b, cat = random_batch(cfg, B=64, Sn=4, seed=92, test=True)
    # histories drawn from the best items, so that exclusion changes the lists
    m = model(cfg, cat, p)
    ref = orc.forward(p, cat, b, 8)
    best = orc.topk_ids(orc.all_item_scores(p, cat, ref["u_t"]), 12)
    b["hist_i"][:, :6] = best[:, ::2]
    b["sl"] = np.maximum(b["sl"], 6)
    b["hist_i"] = np.where(np.arange(cfg["Ls"])[None, :] < b["sl"][:, None], b["hist_i"], 0)
    b["hist_t"] = np.where(b["hist_t"] > 0, b["hist_t"], np.float32(0.5)).astype(np.float32)
    b["hist_t"] = np.where(np.arange(cfg["Ls"])[None, :] < b["sl"][:, None], b["hist_t"], 0).astype(np.float32)
    ref = orc.forward(p, cat, b, 8)
    scores = orc.all_item_scores(p, cat, ref["u_t"])
    hist = history_sets(b)
    rng = np.random.RandomState(93)
    lists = [np.concatenate([best[r, 1::3], rng.randint(-5, 900, 7), best[r, 1:2]]) for r in range(64)]  # repeats, out of range
    for exclude, sets in (("history", hist), (lists, [set(x[(x >= 0) & (x < 800)].tolist()) for x in lists])):
        k = 20
        ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), k, exclude=exclude))
        for r in range(64):
            assert not (set(ids[r].tolist()) & sets[r]), r
        masked = scores.copy()
        for r in range(64):
            masked[r, list(sets[r])] = -np.inf
        want, ws, clear = _oracle_topk(masked, k)
        assert clear.sum() > 40
        assert np.array_equal(ids[clear], want[clear])
        _check_order(ids, sc)
    # fewer eligible items than K
    cfg = make_config(U=20, I=30, C=3, d=64)
    p = p32(random_params(cfg, seed=94))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=95, test=True)
    m = model(cfg, cat, p)
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 40, exclude="history"))
    for r, h in enumerate(history_sets(b)):
        n = 30 - len(h)
        assert np.all(ids[r, n:] == -1) and np.all(sc[r, n:] == -np.inf)
        assert set(ids[r, :n].tolist()) == set(range(30)) - h
    _check_order(ids, sc)
    # the padding of the windows (item 0 past sl / sl_new) is not history: item 0, made the best item, stays first
    p["item_b"][0] = 1000.0
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    ids, _ = (host(t) for t in m.recommend(batch_tuple(b, True), 5, exclude="history"))
    padded = [r for r, h in enumerate(history_sets(b)) if 0 not in h and b["sl"][r] < cfg["Ls"]]
    assert padded
    assert np.all(ids[padded, 0] == 0)


def _avoid(b, item):
    """keep an item out of the batch's inputs (its row is poisoned: u_t must stay finite)"""
    for k in ("i", "j", "hist_i", "hist_i_new"):
        b[k] = np.where(b[k] == item, item + 1, b[k])


def test_topk_nan_item_never_selected():
    cfg = make_config(U=20, I=400, C=7, d=128)
    p = p32(random_params(cfg, seed=101))
    b, cat = random_batch(cfg, B=48, Sn=2, seed=102, test=True)
    _avoid(b, 7)
    p["item_emb"][7] = np.nan
    m = model(cfg, cat, p)
    for k in (1, 50, 256):
        ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), k))
        assert not np.any(ids == 7) and np.all(np.isfinite(sc))
        _check_order(ids, sc)
    # with fewer finite items than K the NaN item comes last, before the padding
    cfg = make_config(U=20, I=20, C=3, d=64)
    p = p32(random_params(cfg, seed=103))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=104, test=True)
    _avoid(b, 7)
    p["item_emb"][7] = np.nan
    m = model(cfg, cat, p)
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 25))
    assert np.all(ids[:, 19] == 7) and np.all(np.isnan(sc[:, 19]))
    assert np.all(ids[:, 20:] == -1)


def _case():
    cfg = make_config(U=61, I=1501, C=9, d=128)
    p = p32(random_params(cfg, seed=111))
    b, cat = random_batch(cfg, B=48, Sn=3, seed=112, test=True)
    return cfg, p, b, cat


def _shard_worker(rank, world, out_dir):
    from tlsan_amd.dist import ShardedModel
    cfg, p, b, cat = _case()
    m = ShardedModel(cfg, cat, device="cuda:0")
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    n = len(b["u"]) // world
    part = {k: v[rank * n:(rank + 1) * n] for k, v in b.items()}
    lists = [np.array([r, 3 * r + 1, 1400, 1400, -2]) for r in range(rank * n, (rank + 1) * n)]
    res = {}
    for name, ex in (("none", None), ("history", "history"), ("lists", lists)):
        ids, sc = m.recommend(batch_tuple(part, True), 30, exclude=ex)
        res[name + "_ids"], res[name + "_sc"] = host(ids), host(sc)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)


def test_sharded_recommend_matches_model(tmp_path):
    world = 2
    run_ranks(_shard_worker, world, str(tmp_path))
    cfg, p, b, cat = _case()
    m = model(cfg, cat, p)
    lists = [np.array([r, 3 * r + 1, 1400, 1400, -2]) for r in range(len(b["u"]))]
    got = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    for name, ex in (("none", None), ("history", "history"), ("lists", lists)):
        ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 30, exclude=ex))
        gi = np.concatenate([g[name + "_ids"] for g in got])
        gs = np.concatenate([g[name + "_sc"] for g in got])
        assert np.array_equal(gi, ids), name
        assert np.array_equal(gs.view(np.int32), sc.view(np.int32)), name


def test_driver_writes_recommendations(tmp_path):
    from tlsan_amd.input import DataInputTest, load_packed
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "30",
                        "--eval_freq", "1000", "--quiet", "--recommend_k", "20"], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(os.path.join(out, "recommend_top20.npz"))
    _, test_set, (U, I, _), _ = load_packed(ds)
    n = len(test_set)
    assert z["ids"].shape == (n, 20) and z["scores"].shape == (n, 20) and z["user"].shape == (n,)
    assert z["ids"].min() >= 0 and z["ids"].max() < I
    row = 0
    for _, batch in DataInputTest(test_set, 128, 10):
        u, _, _, hist_i, hist_new, _, sl, sl_new, _ = batch
        hist_new = np.asarray(hist_new).reshape(len(u), -1)
        for q in range(len(u)):
            h = set(np.asarray(hist_i)[q, :sl[q]].tolist()) | set(hist_new[q, :sl_new[q]].tolist())
            assert not (set(z["ids"][row].tolist()) & h), row
            assert z["user"][row] == u[q]
            row += 1
    assert row == n
    _check_order(z["ids"], z["scores"])

"""GPU tests of the scoped lists (tlsan_eval_topk_scoped / tlsan_similar_topk_scoped, recommend's within= / category=,
similar_items' within= / same_category=): exactly the selection of tests/scope_ref.py from the model's own scores
(score_candidates), against the fp64 oracle, the equivalences with the plain and the exclusion paths bit for bit, the
order's corner cases, the launch geometry at 270 000 items under lazy L2 and bf16 tables, the diversified form, the
similar-items form, the state, and the driver's three flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests import rerank_ref, scope_ref as ref, similar_ref
from tests.helpers import (batch_tuple, bits, history_sets, host, lazy_model, make_config, model, p32, random_batch,
                           random_params)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I0, B0 = 700, 77
FILTERS = ("A", "C", "A+C")
WITHIN_A = np.arange(0, I0, 3)                      # 234 items


def _last_cate(b, cat):
    """numpy's last_item_categories"""
    out = np.full(len(b["u"]), -1, np.int64)
    for r in range(len(out)):
        if b["sl_new"][r] > 0:
            out[r] = cat[b["hist_i_new"][r, b["sl_new"][r] - 1]]
        elif b["sl"][r] > 0:
            out[r] = cat[b["hist_i"][r, b["sl"][r] - 1]]
    return out


def _same(a, b):
    """float32 arrays equal in bits, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _base(d=64, H=8):
    cfg = make_config(U=60, I=I0, C=13, d=d, H=H)
    p = p32(random_params(cfg, seed=51))
    b, cat = random_batch(cfg, B=B0, Sn=3, seed=52, test=True)
    return cfg, p, b, cat


def _filter_args(m, name, tup):
    """recommend's keywords of a filter"""
    kw = {}
    if "A" in name:
        kw["within"] = m.item_scope(items=WITHIN_A)
    if "C" in name:
        kw["category"] = m.last_item_categories(tup)
    return kw


def _filter_mask(name, b, cat, exclude=None):
    return ref.mask_of(B0, I0, within=WITHIN_A if "A" in name else None, category=_last_cate(b, cat) if "C" in name else None,
                       item_cate=cat, exclude=exclude)


@pytest.fixture(scope="module")
def base64():
    cfg, p, b, cat = _base()
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    return m, b, cat, tup, host(m.score_candidates(tup, np.tile(np.arange(I0), (B0, 1))))


def test_last_item_categories_on_the_device(base64):
    m, b, cat, tup, _ = base64
    assert host(m.last_item_categories(tup)).tolist() == _last_cate(b, cat).tolist()


# ---- 1. exact: the reference's selection from the model's own scores
@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (64, 4), (128, 16), (128, 4)])
def test_scoped_lists_are_the_selection_from_the_models_scores(d, H):
    cfg, p, b, cat = _base(d, H)
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    sc_all = host(m.score_candidates(tup, np.tile(np.arange(I0), (B0, 1))))
    assert sc_all.dtype == np.float32
    for name in FILTERS:
        kw = _filter_args(m, name, tup)
        for exclude, sets in ((None, None), ("history", history_sets(b))):
            ok = _filter_mask(name, b, cat, sets)
            for k in (1, 20, 100):
                ids, sc = (host(t) for t in m.recommend(tup, k, exclude=exclude, **kw))
                want_ids, want_sc = ref.topk(sc_all, ok, k)
                assert ids.dtype == np.int32 and np.array_equal(ids, want_ids), (name, exclude, k)
                assert _same(sc, want_sc), (name, exclude, k)
                if k == 100 and "C" in name:
                    assert (ids[:, -1] == -1).all()             # every row of C and A+C is short


# ---- 2. against the fp64 oracle
def _oracle_scoped(scores, ok, k):
    """the oracle's k best eligible ids, their scores, and the rows on which they are unambiguous at fp32 resolution"""
    masked = np.where(ok, scores, -np.inf)
    ids = orc.topk_ids(masked, k + 1)
    s = np.take_along_axis(masked, ids, 1)
    with np.errstate(invalid="ignore"):
        clear = np.all(s[:, :k] - s[:, 1:k + 1] > 1e-4, 1)      # (a row short of k: -inf - -inf is NaN, not clear)
    return ids[:, :k], s[:, :k], clear


@pytest.mark.parametrize("d", [64, 128, 256])
def test_scoped_lists_match_the_oracle(d):
    cfg, p, b, cat = _base(d, 8)
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    scores = orc.all_item_scores(p, cat, orc.forward(p, cat, b, 8)["u_t"])
    for name in FILTERS:
        kw = _filter_args(m, name, tup)
        ok = _filter_mask(name, b, cat)
        n_ok = ok.sum(1)
        for k in (1, 10, 20):
            ids, sc = (host(t) for t in m.recommend(tup, k, **kw))
            want, ws, clear = _oracle_scoped(scores, ok, k)
            full = n_ok >= k
            print("filter %s k %d: %d rows full and clear" % (name, k, int((clear & full).sum())))
            assert (clear & full).sum() >= (35 if (name, k) == ("A+C", 20) else 70), (name, k, int((clear & full).sum()))
            rows = clear & full
            assert np.array_equal(ids[rows], want[rows]), (name, k)
            assert np.abs(sc[rows] - ws[rows]).max() < 1e-4, (name, k)
            for r in np.nonzero(~full)[0]:                       # a short row: exactly its eligible set, then the padding
                assert (ids[r] >= 0).sum() == n_ok[r] and np.all(ids[r, n_ok[r]:] == -1), (name, k, r)
                assert set(ids[r, :n_ok[r]].tolist()) == set(np.nonzero(ok[r])[0].tolist()), (name, k, r)
                assert np.all(sc[r, n_ok[r]:] == -np.inf)
        if name == "A+C":
            assert (n_ok < 20).any() and n_ok.min() >= 10


# ---- 3. equivalences, bit for bit
def _equal(a, b):
    a, b = [host(t) for t in a], [host(t) for t in b]
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1])


def test_equivalences(base64):
    m, b, cat, tup, _ = base64
    everything = m.item_scope(mask=np.ones(I0, bool))
    anything = np.full(B0, -1)
    c_rows = _last_cate(b, cat)
    for k in (1, 20, 100):
        plain = m.recommend(tup, k)
        assert _equal(m.recommend(tup, k, within=everything), plain)
        assert _equal(m.recommend(tup, k, category=anything), plain)
        assert _equal(m.recommend(tup, k, within=everything, category=anything, exclude="history"),
                      m.recommend(tup, k, exclude="history"))
        outside = np.setdiff1d(np.arange(I0), WITHIN_A)
        assert _equal(m.recommend(tup, k, within=m.item_scope(items=WITHIN_A)), m.recommend(tup, k, exclude=[outside] * B0))
        others = [np.nonzero(cat != c)[0] if c >= 0 else np.zeros(0, np.int64) for c in c_rows]
        assert _equal(m.recommend(tup, k, category=c_rows), m.recommend(tup, k, exclude=others))


# ---- 4. order
def _avoid(b, item):
    for k in ("i", "j", "hist_i", "hist_i_new"):
        b[k] = np.where(b[k] == item, item + 1, b[k])


def test_order_of_ties_and_nan_inside_the_scope():
    cfg = make_config(U=20, I=300, C=5, d=64)
    p = p32(random_params(cfg, seed=71))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=72, test=True)
    tied = np.arange(100, 300, 5)[:40]             # 40 items, bit-identical rows, far ahead of the rest
    p["item_emb"][tied] = p["item_emb"][tied[0]]
    p["item_b"][tied] = 1000.0
    cat[tied] = cat[tied[0]]
    lead = np.array([3, 17, 41, 77, 99])
    p["item_b"][lead] = 2000.0 + 100.0 * np.arange(5)
    m = model(cfg, cat, p)
    inside = tied[1::2]                             # half of the tied group, and three of the five leaders
    scope = m.item_scope(items=np.concatenate([inside, lead[[0, 2, 4]], np.arange(1, 100, 7)]))     # (no other leader)
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 10, within=scope))
    assert np.all(ids[:, :3] == lead[[4, 2, 0]][None, :])
    assert np.all(ids[:, 3:] == inside[:7][None, :])            # the tie straddles K: its 7 lowest ids inside the scope
    assert np.all(sc[:, 3:] == sc[:, 3:4])
    # a NaN score inside the scope ranks last, before the padding
    cfg = make_config(U=20, I=40, C=3, d=64)
    p = p32(random_params(cfg, seed=103))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=104, test=True)
    _avoid(b, 7)
    p["item_emb"][7] = np.nan
    m = model(cfg, cat, p)
    scope = m.item_scope(items=[2, 7, 9, 30, 39])
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 8, within=scope))
    assert np.all(np.sort(ids[:, :4], 1) == np.array([2, 9, 30, 39])[None, :]) and np.all(np.isfinite(sc[:, :4]))
    assert np.all(ids[:, 4] == 7) and np.all(np.isnan(sc[:, 4]))
    assert np.all(ids[:, 5:] == -1) and np.all(sc[:, 5:] == -np.inf)


# ---- 5. geometry and selection pressure
BIG = 270000


def _scattered(n, seed):
    """n distinct ids of the big table, item 0 and item BIG - 1 among them (n = 1: the last item alone)"""
    if n == 0:
        return np.zeros(0, np.int64)
    if n == 1:
        return np.array([BIG - 1])
    mid = np.random.RandomState(seed).choice(np.arange(1, BIG - 1), n - 2, replace=False)
    return np.sort(np.concatenate([[0], mid, [BIG - 1]]))


@pytest.mark.parametrize("table_dtype", ["bf16", "f32"])
def test_geometry_and_selection_pressure(table_dtype):
    import torch
    cfg, m = lazy_model(BIG, table_dtype, seed=61)
    b, _ = random_batch(cfg, B=2000, Sn=3, seed=63, test=True)
    few = {k: v[:45] for k, v in b.items()}

    def check(rows, ids_in):
        tup, n = batch_tuple(rows, True), len(rows["u"])
        scope = m.item_scope(items=ids_in)
        assert scope.count == len(ids_in)
        if len(ids_in):
            s = host(m.score_candidates(tup, np.tile(ids_in, (n, 1))))
            pos, sc_ref = ref.topk(s, np.ones_like(s, bool), 256)          # the K best are a prefix of the 256 best
            id_ref = np.where(pos >= 0, ids_in[np.maximum(pos, 0)], -1).astype(np.int32)
        else:
            id_ref, sc_ref = np.full((n, 256), -1, np.int32), np.full((n, 256), -np.inf, np.float32)
        for k in (1, 64, 256):
            ids, sc = (host(t) for t in m.recommend(tup, k, within=scope))
            assert np.array_equal(ids, id_ref[:, :k]), (len(ids_in), k)
            assert _same(sc, sc_ref[:, :k]), (len(ids_in), k)

    for n in (0, 1, 15, 64, 257):
        check(few, _scattered(n, 70 + n))
    # scores rising with the id: every later item beats the threshold and the buffers overflow (2 000 rows: 17 slices,
    # two rounds for some of them)
    ids5k = _scattered(5000, 75)
    m.item_b[torch.as_tensor(ids5k).to(m.device)] = torch.as_tensor((10.0 * ids5k).astype(np.float32)).to(m.device)
    check(b, ids5k)


def test_empty_scope_and_empty_category():
    cfg = make_config(U=20, I=300, C=5, d=128)
    p = p32(random_params(cfg, seed=91))
    b, cat = random_batch(cfg, B=20, Sn=2, seed=92, test=True)
    cat = (cat % 4).astype(np.int32)                # no item has category 4
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    for kw in (dict(within=m.item_scope(items=[])), dict(category=np.full(20, 4)), dict(within=m.item_scope(categories=[4])),
               dict(within=m.item_scope(items=np.nonzero(cat == 1)[0]), category=np.full(20, 2))):
        for k in (1, 64, 256):
            ids, sc = (host(t) for t in m.recommend(tup, k, **kw))
            assert ids.shape == (20, k) and np.all(ids == -1) and np.all(sc == -np.inf), (list(kw), k)
    some = np.where(np.arange(20) % 2 == 0, 4, -1)  # every other row wants the empty category
    ids = host(m.recommend(tup, 5, category=some)[0])
    assert np.all(ids[::2] == -1) and np.array_equal(ids[1::2], host(m.recommend(tup, 5)[0])[1::2])


def test_an_index_outside_the_table_is_never_read_as_a_row_nor_selected(base64):
    """a caller's bad list through the C calls (ItemScope refuses such ids): the holes count as if they were not there"""
    import torch
    from tlsan_amd import model as M
    m, _, _, tup, _ = base64
    good = np.array([0, 5, 6, 300, 699])
    listed = np.array([-1, 0, 5, -2 ** 31, 6, I0, 300, 2 ** 31 - 1, 699, 100000])
    sub = (torch.as_tensor(listed.astype(np.int32)).to(m.device), len(listed))
    scope = m.item_scope(items=good)
    _, _, ut, db = m.forward(tup, is_test=True, want_u_t=True)
    for k in (1, 3, 20):
        got = M.scoped_topk(m.lib, m.dims, m.cparams, ut, db.B, k, (None, None), sub, None, 1, 0, m._topk_workspace, m._stream())
        assert _equal(got, m.recommend(tup, k, within=scope)), k
    qids = torch.as_tensor(np.array([5, 17, 699], np.int32)).to(m.device)
    vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, qids, 1, 0, m._stream())
    for metric in ("cosine", "dot"):
        got = M.scoped_similar_topk(m.lib, m.dims, m.cparams, vec, inv, qids, 4, M.SIMILAR_METRICS[metric], (None, None), sub, None,
                                    1, 0, m._topk_workspace, m._stream())
        assert _equal(got, m.similar_items([5, 17, 699], 4, metric=metric, within=scope)), metric


# ---- 6. diversified
def test_diversified_lists_come_from_the_scoped_pool(base64):
    import torch
    from tlsan_amd import model as M
    m, b, cat, tup, _ = base64
    scope = m.item_scope(items=WITHIN_A)
    K, N, theta, cap, d = 10, 64, 0.3, 2, 64
    ids, sc = (host(t) for t in m.recommend(tup, K, within=scope, per_category=cap, diversity=theta, pool=N))
    pid, psc = m.recommend(tup, N, within=scope)
    vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, pid.reshape(-1).contiguous(), 1, 0, m._stream())
    torch.cuda.synchronize()
    pid_h, psc_h = host(pid), host(psc)
    assert np.isin(pid_h, WITHIN_A).all() and (pid_h >= 0).all()
    w, inv = host(vec).reshape(B0, N, -1), host(inv).reshape(B0, N)
    pc = np.asarray(cat)[pid_h]
    for r in range(B0):                             # teacher-forced in fp64, as tests/test_gpu_rerank.py checks a list
        picks = rerank_ref.positions(pid_h[r], ids[r])
        regret, was, more = rerank_ref.replay(pid_h[r], psc_h[r], w[r], inv[r], pc[r], theta, cap, picks)
        assert was.all() and np.all(regret <= rerank_ref.tau(d)), (r, float(regret.max()))
        assert len(picks) == K or not more, r
        assert np.array_equal(bits(sc[r, :len(picks)]), bits(psc_h[r, picks])), r
        assert np.bincount(pc[r, picks]).max() <= cap
    # theta = 0: integer logic only, the reference's own list
    ids0, sc0 = (host(t) for t in m.recommend(tup, K, within=scope, per_category=cap, pool=N))
    for r in range(B0):
        picks = rerank_ref.select(pid_h[r], psc_h[r], w[r], inv[r], pc[r], K, 0.0, cap)
        assert ids0[r, :len(picks)].tolist() == pid_h[r, picks].tolist() and np.all(ids0[r, len(picks):] == -1), r
        assert np.array_equal(bits(sc0[r, :len(picks)]), bits(psc_h[r, picks])), r


# ---- 7. similar_items
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_scoped_similar_items(base64, metric):
    m, _, cat, _, _ = base64
    w = similar_ref.item_matrix(host(m.item_emb.float()), host(m.cate_emb.float()), cat)
    qids = np.concatenate([np.arange(0, I0, 41), [1, 2, 699, 3]])
    s, tol = similar_ref.scores(w, qids, metric), similar_ref.tolerance(w, qids, metric)
    inside = np.zeros(I0, bool)
    inside[WITHIN_A] = True
    same = np.asarray(cat)[None, :] == np.asarray(cat)[qids][:, None]
    scope = m.item_scope(items=WITHIN_A)
    for kw, ok in ((dict(same_category=True), same), (dict(within=scope), np.tile(inside, (len(qids), 1))),
                   (dict(within=scope, same_category=True), same & inside[None, :])):
        ok = ok & similar_ref.eligible(I0, qids)
        for k in (5, 64, 256):
            ids, sc = (host(t) for t in m.similar_items(qids, k, metric=metric, **kw))
            assert ids.shape == (len(qids), k) and ids.dtype == np.int32
            similar_ref.check_lists(ids, sc, s, ok, tol)
            assert not np.any(ids == qids[:, None])                     # the query is never in its own list
    # with an exclusion list, and the scope of everything: the plain lists bit for bit
    excl = [[int(q) // 2, 3, 6, 9] for q in qids]
    ids, sc = (host(t) for t in m.similar_items(qids, 20, metric=metric, exclude=excl, within=scope))
    similar_ref.check_lists(ids, sc, s, inside[None, :] & similar_ref.eligible(I0, qids, excl), tol)
    assert _equal(m.similar_items(qids, 20, metric=metric, within=m.item_scope(mask=np.ones(I0, bool))),
                  m.similar_items(qids, 20, metric=metric))


# ---- 8. state and arguments
def test_state_is_read_not_changed_and_bad_arguments_are_refused():
    import torch
    cfg = make_config(U=40, I=500, C=7, d=128, H=8)
    tb, cat = random_batch(cfg, B=64, Sn=3, seed=72)
    b, _ = random_batch(cfg, B=30, Sn=3, seed=73, test=True)
    m = model(cfg, cat, random_params(cfg, seed=71), l2_mode="lazy")
    for _ in range(3):
        m.train(None, batch_tuple(tb), 1.0)
    tup = batch_tuple(b, True)
    scope = m.item_scope(items=np.arange(0, 500, 3))
    m.recommend(tup, 5, within=scope)                            # (what the last step owed lands with the first call)
    P = m.table_scale()
    assert P != 1.0
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.cate_emb, m.item_b, m.dense)]
    before = snap()
    m.recommend(tup, 20, within=scope, category=m.last_item_categories(tup), exclude="history")
    m.recommend(tup, 5, within=scope, per_category=1, diversity=0.5)
    m.similar_items(np.arange(0, 500, 23), 10, within=scope, same_category=True)
    m.similar_items(np.arange(0, 500, 23), 10, metric="dot", same_category=True)
    after = snap()
    assert m.table_scale() == P
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, after))
    other = model(make_config(U=40, I=400, C=7, d=128, H=8), cat[:400]).item_scope(items=[1])
    for kw in (dict(within=[1, 2, 3]), dict(within=other), dict(category=np.full(30, 7)), dict(category=np.zeros(29, np.int64)),
               dict(category=np.zeros(30, np.float32)), dict(within=scope, pool=64)):
        with pytest.raises(ValueError):
            m.recommend(tup, 5, **kw)
    for kw in (dict(within=[1, 2, 3]), dict(within=other)):
        with pytest.raises(ValueError):
            m.similar_items([1, 2], 5, **kw)
    for kw in (dict(items=[500]), dict(items=[-1]), dict(mask=np.ones(499, bool))):
        with pytest.raises(ValueError):
            m.item_scope(**kw)
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, snap()))


# ---- 9. the driver
@pytest.mark.parametrize("flags", [("--recommend_categories", "3,7,12", "--similar_k", "5", "--similar_same_category", "1"),
                                   ("--recommend_same_category", "1")])
def test_driver_writes_scoped_lists(tmp_path, flags):
    from tlsan_amd.input import DataInputTest, load_packed
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "30",
                        "--eval_freq", "1000", "--quiet", "--recommend_k", "10", "--recommend_exclude", "none"] + list(flags),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cat = np.load(ds)["item_cate_list"].astype(np.int64)
    _, test_set, (_, I, _), _ = load_packed(ds)
    z = np.load(os.path.join(out, "recommend_top10.npz"))             # the lists keep their files and formats
    ids = z["ids"]
    assert ids.shape == (len(test_set), 10) and z["scores"].shape == ids.shape and ids.max() < I
    if "--recommend_categories" in flags:
        inside = int(np.isin(cat, [3, 7, 12]).sum())
        assert 0 < inside and np.all((ids >= 0).sum(1) == min(10, inside))
        assert np.isin(cat[ids[ids >= 0]], [3, 7, 12]).all()
        s = np.load(os.path.join(out, "similar-5.npz"))
        assert s["ids"].shape == (I, 5)
        same = np.where(s["ids"] >= 0, cat[np.maximum(s["ids"], 0)], cat[:, None])
        assert np.all(same == cat[:, None]) and not np.any(s["ids"] == np.arange(I)[:, None])
        assert np.all((s["ids"] >= 0).sum(1) == np.minimum(5, np.bincount(cat, minlength=cat.max() + 1)[cat] - 1))
    else:
        row = 0
        for _, batch in DataInputTest(test_set, 128, 10):
            _, _, _, hist_i, hist_new, _, sl, sl_new, _ = batch
            hist_new = np.asarray(hist_new).reshape(len(sl), -1)
            for q in range(len(sl)):
                last = hist_new[q, sl_new[q] - 1] if sl_new[q] > 0 else np.asarray(hist_i)[q, sl[q] - 1]
                got = ids[row][ids[row] >= 0]
                assert len(got) == min(10, int((cat == cat[last]).sum())) and np.all(cat[got] == cat[last]), row
                row += 1
        assert row == len(test_set)

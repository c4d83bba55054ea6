"""GPU tests of the boosted lists (tlsan_eval_topk_scoped_boost / tlsan_eval_topk_lists_boost, recommend's boost= and
boost_weight=).  The oracle of every case: score_candidates over all items gives the model's scores s bit for bit,
tests/boost_ref.py forms s' = fl(s + t) and selects, and the ids and the score bits must be EQUAL.  Small tables: 4099 items
(no multiple of 256: several rounds and slices), 23 categories, 37 rows (no multiple of 16)."""
import numpy as np
import pytest

from tests import boost_ref as ref, lists_ref, rerank_ref, scope_ref
from tests.helpers import (batch_tuple, bits, history_sets, host, lazy_model, make_config, model, p32, random_batch,
                           random_params)

pytestmark = pytest.mark.gpu

I0, C0, B0 = 4099, 23, 37
ALL = np.arange(I0)


def _same(a, b):
    """float32 arrays equal in bits, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _equal(a, b):
    a, b = [host(t) for t in a], [host(t) for t in b]
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1])


def _case(d=64, H=8):
    cfg = make_config(U=60, I=I0, C=C0, d=d, H=H)
    p = p32(random_params(cfg, seed=61))
    b, cat = random_batch(cfg, B=B0, Sn=3, seed=62, test=True)
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    return m, b, cat, tup, host(m.score_candidates(tup, np.tile(ALL, (B0, 1))))


@pytest.fixture(scope="module")
def base64():
    return _case()


def _random_boost(sc_all, seed):
    """a boost of the scale of the scores' spread"""
    return (np.random.RandomState(seed).randn(I0) * sc_all.std()).astype(np.float32)


def _check(m, tup, sc_all, k, boost, weight=None, ok=None, **kw):
    """recommend(boost=, boost_weight=, **kw) against the reference on the eligible (row, item) pairs `ok` (None: all)"""
    got = m.recommend(tup, k, boost=boost, boost_weight=weight, **kw)
    ids, sc = (host(t) for t in got)
    adj = ref.adjusted(sc_all, boost, None if weight is None else np.asarray(weight, np.float32))
    want_ids, want_sc = ref.topk(adj, ALL, k, None if ok is None else ~ok)
    assert ids.dtype == np.int32 and sc.dtype == np.float32
    assert np.array_equal(ids, want_ids), (k, kw.keys())
    assert _same(sc, want_sc), (k, kw.keys())
    return ids, sc, adj


# ---- sizes
@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8)])
def test_boosted_lists_are_the_selection_from_the_adjusted_scores(d, H):
    m, b, cat, tup, sc_all = _case(d, H)
    boost = _random_boost(sc_all, 7)
    moved = 0
    for k in (1, 10, 256):
        ids, _, _ = _check(m, tup, sc_all, k, boost)
        moved += int((ids != host(m.recommend(tup, k)[0])).sum())
    assert moved > 0                                      # the boost changes the lists: the test is not about the plain path
    held = m.item_boost(boost)                            # a holder, reused across calls
    assert _equal(m.recommend(tup, 10, boost=held), m.recommend(tup, 10, boost=boost))


# ---- a zero boost
def test_zero_boost_is_the_call_without_one(base64):
    m, b, cat, tup, sc_all = base64
    zero = np.zeros(I0, np.float32)
    scope = m.item_scope(items=ALL[::6])
    idx = m.category_index()
    c = host(m.last_item_categories(tup)).astype(np.int64)
    for k in (1, 10, 256):
        for kw in (dict(), dict(exclude="history"), dict(within=scope), dict(category=c), dict(category=c, index=idx)):
            assert _equal(m.recommend(tup, k, boost=zero, **kw), m.recommend(tup, k, **kw)), (k, kw.keys())
    assert _equal(m.recommend(tup, 10, boost=zero, boost_weight=np.linspace(-3, 3, B0)), m.recommend(tup, 10))


# ---- ties
@pytest.mark.parametrize("value,k", [(2.0 ** 20, 64), (2.0 ** 24, 256)])
def test_ties_come_in_id_order(base64, value, k):
    m, b, cat, tup, sc_all = base64
    lifted = np.unique(np.concatenate([[0, I0 - 1], np.random.RandomState(3).choice(I0, 300, replace=False)]))
    boost = np.zeros(I0, np.float32)
    boost[lifted] = value
    ids, sc, adj = _check(m, tup, sc_all, k, boost)
    assert np.isin(ids, lifted).all()                     # the lifted items fill every list
    tie = sc[:, :-1] == sc[:, 1:]
    print("boost %g: %d tied neighbours in %d rows, %d distinct values among the lifted" %
          (value, int(tie.sum()), int(tie.any(1).sum()), len(np.unique(adj[:, lifted]))))
    assert tie.any(1).all()                               # every row really holds equal s' at different ids ...
    assert (ids[:, :-1][tie] < ids[:, 1:][tie]).all()     # ... and they come in id order
    if value == 2.0 ** 24:      # the grid is 1 below 2^24 and 2 above it: a row's 256 entries share a handful of values
        assert (tie.sum(1) >= k - 1 - 2 * np.ceil(np.abs(sc_all).max(1)) - 1).all()


# ---- special values
def test_minus_inf_buries_and_nan_ranks_last(base64):
    m, b, cat, tup, sc_all = base64
    twelve = np.array([0, 5, 255, 256, 257, 1000, 2048, 3000, 4000, 4096, 4097, I0 - 1])
    buried, broken = twelve[[1, 4, 9]], twelve[[2, 11]]
    boost = _random_boost(sc_all, 11)
    boost[buried] = -np.inf
    boost[broken] = np.nan
    scope = m.item_scope(items=twelve)
    ok = scope_ref.mask_of(B0, I0, within=twelve)
    ids, sc, _ = _check(m, tup, sc_all, 16, boost, within=scope, ok=ok)
    assert (ids[:, 12:] == -1).all() and (sc[:, 12:] == -np.inf).all()            # 12 items, then the padding
    assert np.isfinite(sc[:, :7]).all() and not np.isin(ids[:, :7], np.concatenate([buried, broken])).any()
    assert np.array_equal(ids[:, 7:10], np.tile(buried, (B0, 1))) and (sc[:, 7:10] == -np.inf).all()   # -inf: a score, by id
    assert np.array_equal(ids[:, 10:12], np.tile(broken, (B0, 1))) and np.isnan(sc[:, 10:12]).all()     # NaN last
    ids, sc, _ = _check(m, tup, sc_all, 5, boost, within=scope, ok=ok)              # K below the finite count: none of them
    assert np.isfinite(sc).all()
    # over the whole table a buried set never shows up while finite items are left, and 0 * -inf = NaN ranks last
    boost = np.zeros(I0, np.float32)
    boost[::2] = -np.inf
    ids, sc, _ = _check(m, tup, sc_all, 256, boost)
    assert (ids % 2 == 1).all() and np.isfinite(sc).all()
    w = np.ones(B0, np.float32)
    w[::5] = 0.0
    ids, sc, _ = _check(m, tup, sc_all, 10, boost, weight=w)
    assert (ids % 2 == 1).all()


# ---- row weights
def test_row_weights(base64):
    m, b, cat, tup, sc_all = base64
    boost = _random_boost(sc_all, 13)
    w = np.random.RandomState(14).randn(B0).astype(np.float32) * 2
    w[0:12:3], w[1:12:3], w[2:12:3] = 0.0, 1.0, -1.0
    for k in (1, 10, 256):
        ids, sc, _ = _check(m, tup, sc_all, k, boost, weight=w)
        plain = [host(t) for t in m.recommend(tup, k)]
        one = [host(t) for t in m.recommend(tup, k, boost=boost)]
        assert np.array_equal(ids[w == 0], plain[0][w == 0]) and _same(sc[w == 0], plain[1][w == 0])   # weight 0: unboosted
        assert np.array_equal(ids[w == 1], one[0][w == 1]) and _same(sc[w == 1], one[1][w == 1])       # weight 1: no weight
    # a row's result is its own: the same rows alone, and a weight tensor on the device
    import torch
    few = tuple(x[:5] for x in tup)
    assert _equal(m.recommend(few, 10, boost=boost, boost_weight=torch.as_tensor(w[:5]).to(m.device)),
                  [t[:5] for t in m.recommend(tup, 10, boost=boost, boost_weight=w)])


# ---- state and dtype
@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
def test_lazy_l2_and_bf16_tables(table_dtype):
    cfg, m = lazy_model(I0, table_dtype, seed=41)            # d = 256, P != 1 after two lazy-L2 steps
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=43, test=True)
    tup = batch_tuple(b, True)
    sc_all = host(m.score_candidates(tup, np.tile(ALL, (B0, 1))))
    boost = _random_boost(sc_all, 17)
    w = np.random.RandomState(18).rand(B0).astype(np.float32)
    for k in (10, 256):
        _check(m, tup, sc_all, k, boost)
        _check(m, tup, sc_all, k, boost, weight=w, exclude="history", ok=scope_ref.mask_of(B0, I0, exclude=history_sets(b)))


# ---- composition
def test_composes_with_exclusion_scope_and_category(base64):
    m, b, cat, tup, sc_all = base64
    boost = _random_boost(sc_all, 19)
    w = np.random.RandomState(20).randn(B0).astype(np.float32)
    within = np.random.RandomState(21).choice(I0, 700, replace=False)
    scope = m.item_scope(items=within)
    c = host(m.last_item_categories(tup)).astype(np.int64)
    c[::7] = -1
    sets = history_sets(b)
    lifted = np.concatenate([np.asarray(sorted(s))[:2] for s in sets])       # the boost lifts seen items: they stay out
    boost[lifted] += 100.0
    for k in (10, 256):
        for weight in (None, w):
            _check(m, tup, sc_all, k, boost, weight, exclude="history", ok=scope_ref.mask_of(B0, I0, exclude=sets))
            _check(m, tup, sc_all, k, boost, weight, within=scope, ok=scope_ref.mask_of(B0, I0, within=within))
            _check(m, tup, sc_all, k, boost, weight, category=c, ok=scope_ref.mask_of(B0, I0, category=c, item_cate=cat))
            _check(m, tup, sc_all, k, boost, weight, within=scope, category=c, exclude="history",
                   ok=scope_ref.mask_of(B0, I0, within=within, category=c, item_cate=cat, exclude=sets))


def test_composes_with_a_category_index(base64):
    m, b, cat, tup, sc_all = base64
    boost = _random_boost(sc_all, 23)
    w = np.random.RandomState(24).randn(B0).astype(np.float32)
    rng = np.random.RandomState(25)
    rows = rng.randint(0, C0, (B0, 3))
    rows[rng.rand(B0, 3) < 0.25] = -1
    rows[[3, 20, 36]] = -1                                                      # rows of negatives only: unrestricted
    rows[5] = [7, 7, 7]
    idx = m.category_index()
    off, items = lists_ref.index_of(cat, C0)
    free = (rows < 0).all(1)
    assert free.sum() >= 3
    for exclude, sets in ((None, None), ("history", history_sets(b))):
        ok = lists_ref.union_mask(B0, I0, rows, off, items, exclude=sets)
        ok[free] = scope_ref.mask_of(B0, I0, exclude=sets)[free]
        for k in (10, 256):
            _check(m, tup, sc_all, k, boost, None, category=rows, index=idx, exclude=exclude, ok=ok)
            _check(m, tup, sc_all, k, boost, w, category=rows, index=idx, exclude=exclude, ok=ok)   # the sub-batch's weights
    c = rows[:, 0]
    assert _equal(m.recommend(tup, 10, boost=boost, boost_weight=w, category=c, index=idx),
                  m.recommend(tup, 10, boost=boost, boost_weight=w, category=c))
    within = ALL[::3]
    sidx = m.category_index(within=m.item_scope(items=within))                  # the unrestricted rows scan the index's scope
    ok = lists_ref.union_mask(B0, I0, rows, off, items) & scope_ref.mask_of(B0, I0, within=within)
    ok[free] = scope_ref.mask_of(B0, I0, within=within)[free]
    _check(m, tup, sc_all, 10, boost, w, category=rows, index=sidx, ok=ok)


def test_clustered_index_probing_every_list_is_the_boosted_exact_list(base64):
    from tlsan_amd.cluster import ClusteredIndex
    m, b, cat, tup, sc_all = base64
    boost = _random_boost(sc_all, 27)
    w = np.random.RandomState(28).randn(B0).astype(np.float32)
    cent = np.random.RandomState(29).randn(8, 64).astype(np.float32)
    ci = ClusteredIndex.from_assignment(ALL % 8, cent, device=m.device, item_b=host(m.item_b))
    assert ci.lists == 8 and ci.nonempty == 8
    for k in (10, 256):
        _check(m, tup, sc_all, k, boost, w, index=ci, probes=8)
        _check(m, tup, sc_all, k, boost, None, index=ci, probes=8, exclude="history",
               ok=scope_ref.mask_of(B0, I0, exclude=history_sets(b)))
    # fewer probes: the boosted top k of the probed lists' union (the lists are chosen by the unboosted centroid scores)
    _, _, ut, _ = m.forward(tup, is_test=True, want_u_t=True)
    probed = host(ci.probe(ut, 3, scale=m._scale_vector(ci.lists), bias=ci.list_bias))
    ok = (probed[:, :, None] == (ALL % 8)[None, None, :]).any(1)
    _check(m, tup, sc_all, 10, boost, w, index=ci, probes=3, ok=ok)


def test_diversified_lists_come_from_the_boosted_pool(base64):
    from tlsan_amd import model as M
    m, b, cat, tup, sc_all = base64
    boost = _random_boost(sc_all, 31)
    w = np.random.RandomState(32).rand(B0).astype(np.float32) + 0.5
    K, N, theta, cap, d = 10, 64, 0.3, 2, 64
    ids, sc = (host(t) for t in m.recommend(tup, K, diversity=theta, per_category=cap, pool=N, boost=boost, boost_weight=w))
    pid_h, psc_h = ref.topk(ref.adjusted(sc_all, boost, w), ALL, N)             # the boosted pool, by the reference
    pool = m.recommend(tup, N, boost=boost, boost_weight=w)
    assert np.array_equal(host(pool[0]), pid_h) and _same(host(pool[1]), psc_h)
    vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, pool[0].reshape(-1).contiguous(), 1, 0, m._stream())
    vec, inv = host(vec).reshape(B0, N, -1), host(inv).reshape(B0, N)
    pc = np.asarray(cat)[pid_h]
    for r in range(B0):                             # teacher-forced in fp64 on the boosted pool: the relevance is s''s
        picks = rerank_ref.positions(pid_h[r], ids[r])
        regret, was, more = rerank_ref.replay(pid_h[r], psc_h[r], vec[r], inv[r], pc[r], theta, cap, picks)
        assert was.all() and np.all(regret <= rerank_ref.tau(d)), (r, float(regret.max()))
        assert len(picks) == K or not more, r
        assert np.array_equal(bits(sc[r, :len(picks)]), bits(psc_h[r, picks])), r  # the scores returned are s'
        assert np.bincount(pc[r, picks]).max() <= cap
    ids0, sc0 = (host(t) for t in m.recommend(tup, K, per_category=cap, pool=N, boost=boost, boost_weight=w))
    for r in range(B0):                             # theta = 0: integer logic only, the reference's own list
        picks = rerank_ref.select(pid_h[r], psc_h[r], vec[r], inv[r], pc[r], K, 0.0, cap)
        assert ids0[r, :len(picks)].tolist() == pid_h[r, picks].tolist() and np.all(ids0[r, len(picks):] == -1), r
        assert np.array_equal(bits(sc0[r, :len(picks)]), bits(psc_h[r, picks])), r


# ---- refusals
def test_python_refusals(base64):
    m, b, cat, tup, sc_all = base64
    boost = np.zeros(I0, np.float32)
    other = model(make_config(U=40, I=400, C=7, d=64, H=8), cat[:400] % 7)
    for kw in (dict(boost_weight=np.ones(B0)), dict(boost=np.zeros(I0 - 1, np.float32)), dict(boost=other.item_boost(np.zeros(400))),
               dict(boost=boost, boost_weight=np.ones(B0 + 1)), dict(boost=boost, boost_weight=np.ones((B0, 1))),
               dict(boost=boost, index=m.shortlist_index())):
        with pytest.raises(ValueError):
            m.recommend(tup, 10, **kw)
    assert m.item_boost(items=([0, I0 - 1], 2.0), base=1.0).values.device.type == "cuda"
    want = np.arange(C0, dtype=np.float32)[cat]
    assert np.array_equal(host(m.item_boost(categories=np.arange(C0)).values), want)

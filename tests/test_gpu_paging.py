"""GPU tests of the list cursors (tlsan_eval_topk_scoped_after / tlsan_eval_topk_lists_after / tlsan_dense_topk_after, the
after= of recommend and audience, recommend_deep and audience_deep).  The oracle of every case: score_candidates over all
items gives the model's scores bit for bit, tests/boost_ref.py forms s' where a boost is given, tests/paging_ref.py selects
what lies strictly behind each row's cursor, and the ids and the score bits must be EQUAL.  Small tables: 4099 items (no
multiple of 256: several rounds and slices), 23 categories, 37 rows (no multiple of 16)."""
import numpy as np
import pytest

from tests import audience_ref, boost_ref, lists_ref, paging_ref as ref, scope_ref
from tests.helpers import batch_tuple, bits, history_sets, host, make_config, model, p32, random_batch, random_params

pytestmark = pytest.mark.gpu

I0, C0, B0 = 4099, 23, 37
ALL = np.arange(I0)


def _same(a, b):
    """float32 arrays equal in bits, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _equal(a, b):
    arr = lambda t: t if isinstance(t, np.ndarray) else host(t)
    a, b = [arr(t) for t in a], [arr(t) for t in b]
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


def _walk(m, tup, k, pages, after=None, **kw):
    """`pages` pages of recommend(k, after=) chained through ListCursor.of -> the pages, as host arrays"""
    from tlsan_amd.model import ListCursor
    out = []
    for _ in range(pages):
        got = m.recommend(tup, k, after=after, **kw) if after is not None else m.recommend(tup, k, after=ListCursor.start(B0, m.device), **kw)
        out.append((host(got[0]), host(got[1])))
        after = ListCursor.of(*got)
    return out


def _cat(pages):
    return np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)


def _tiles(m, tup, adj, k, pages, ok=None, walk_ref=True, **kw):
    """the chained pages against the reference's: page by page (walk_ref) and as the head of the exact ranking"""
    got = _walk(m, tup, k, pages, **kw)
    ids, sc = _cat(got)
    assert ids.dtype == np.int32 and sc.dtype == np.float32
    want_ids, want_sc = boost_ref.topk(adj, ALL, k * pages, None if ok is None else ~ok)
    assert np.array_equal(ids, want_ids), (k, pages, kw.keys())
    assert _same(sc, want_sc), (k, pages, kw.keys())
    if walk_ref:
        for j, (g, w) in enumerate(zip(got, ref.walk(adj, ALL, k, pages, None if ok is None else ~ok))):
            assert np.array_equal(g[0], w[0]) and _same(g[1], w[1]), (k, j, kw.keys())
    return got


# ---- tiling
@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8)])
def test_pages_tile_the_exact_ranking(d, H):
    m, b, cat, tup, sc_all = _case(d, H)
    changed = 0
    for k, pages in ((1, 258), (7, 40), (64, 5), (256, 2)):                    # every arm of TOPK_DISPATCH, to a depth past 256
        got = _tiles(m, tup, sc_all, k, pages, walk_ref=pages <= 40)
        head = 256 // k                                                        # the pages one call can still reach
        assert _equal(m.recommend(tup, head * k), _cat(got[:head])), k
        plain = host(m.recommend(tup, k)[0])                                   # the call without after=: page 1 ...
        assert np.array_equal(got[0][0], plain)
        changed += int((got[1][0] != plain).any(1).sum())                      # ... which page 2 is not: the cursor was applied
        if k < 256:
            assert np.array_equal(got[1][0], host(m.recommend(tup, 2 * k)[0])[:, k:]), k      # it is columns K .. 2 K of the deeper call
    assert changed == 4 * B0                                                   # every row's page 2, at every K


# ---- ties
@pytest.mark.parametrize("k", [7, 64])
def test_pages_tile_through_ties(base64, k):
    m, b, cat, tup, sc_all = base64
    lifted = np.unique(np.concatenate([[0, I0 - 1], np.random.RandomState(3).choice(I0, 300, replace=False)]))
    boost = np.zeros(I0, np.float32)
    boost[lifted] = 2.0 ** 24                   # the grid is 2 above 2^24: a row's head is a handful of values
    adj = boost_ref.adjusted(sc_all, boost)
    pages = -(-320 // k)                        # past the lifted items, into the unlifted ones
    got = _tiles(m, tup, adj, k, pages, boost=boost)
    last = np.stack([p[1][:, -1] for p in got[:-1]], 1)
    nxt = np.stack([p[1][:, 0] for p in got[1:]], 1)
    last_id = np.stack([p[0][:, -1] for p in got[:-1]], 1)
    nxt_id = np.stack([p[0][:, 0] for p in got[1:]], 1)
    tie = last == nxt
    print("k %d: %d of %d cursors sit inside a tie group" % (k, int(tie.sum()), tie.size))
    assert tie.any(1).all()                     # in every row some cursor really has a successor of equal s' ...
    assert (last_id[tie] < nxt_id[tie]).all()   # ... at a higher id


# ---- special values
def test_cursors_at_minus_inf_and_nan_entries(base64):
    from tlsan_amd.model import ListCursor
    m, b, cat, tup, sc_all = base64
    twelve = np.array([0, 5, 255, 256, 257, 1000, 2048, 3000, 4000, 4096, 4097, I0 - 1])
    buried, broken = twelve[[1, 4, 9]], twelve[[2, 11]]
    boost = (np.random.RandomState(11).randn(I0) * sc_all.std()).astype(np.float32)
    boost[buried] = -np.inf
    boost[broken] = np.nan
    scope = m.item_scope(items=twelve)
    ok = scope_ref.mask_of(B0, I0, within=twelve)
    adj = boost_ref.adjusted(sc_all, boost)
    got = _tiles(m, tup, adj, 5, 5, ok=ok, within=scope, boost=boost)          # 7 finite, 3 x -inf, 2 x NaN
    assert np.isfinite(got[0][1]).all()
    assert np.isfinite(got[1][1][:, :2]).all() and (got[1][1][:, 2:] == -np.inf).all() and np.array_equal(got[1][0][:, 2:], np.tile(buried, (B0, 1)))
    assert np.array_equal(got[2][0][:, :2], np.tile(broken, (B0, 1))) and np.isnan(got[2][1][:, :2]).all()     # behind a -inf cursor
    assert (got[2][0][:, 2:] == -1).all() and (got[2][1][:, 2:] == -np.inf).all()
    for p in got[3:]:                                                           # empty, and still empty
        assert (p[0] == -1).all() and (p[1] == -np.inf).all()
    got4 = _tiles(m, tup, adj, 4, 4, ok=ok, within=scope, boost=boost)          # cursors at the first -inf and at the last NaN
    assert (got4[1][1][:, -1] == -np.inf).all() and np.isnan(got4[2][1][:, -1]).all() and (got4[3][0] == -1).all()
    got11 = _tiles(m, tup, adj, 11, 3, ok=ok, within=scope, boost=boost)        # a cursor at the first NaN entry
    assert np.isnan(got11[0][1][:, -1]).all() and np.array_equal(got11[1][0][:, 0], np.full(B0, broken[1])) and (got11[1][0][:, 1:] == -1).all()
    # the NaN's payload and the zero's sign of a cursor do not matter
    cur = ListCursor(got11[0][0][:, -1], np.full(B0, 0xFFC00123, np.uint32).view(np.float32))     # a negative NaN with a payload
    assert _equal(m.recommend(tup, 11, after=cur, within=scope, boost=boost), got11[1])
    at = ListCursor(np.full(B0, twelve[3]), np.full(B0, -0.0, np.float32))
    flat = m.recommend(tup, 12, after=at, within=scope, boost=np.where(np.isin(ALL, twelve), -sc_all[0], 0).astype(np.float32))
    assert (host(flat[0])[0] == np.concatenate([twelve[4:], [-1] * 4])).all()      # row 0: every s' is 0, the cursor a -0.0


# ---- mixed depths in one launch
def test_rows_at_different_depths_share_a_launch(base64):
    from tlsan_amd.model import ListCursor
    m, b, cat, tup, sc_all = base64
    sets = history_sets(b)
    within = np.setdiff1d(ALL, ALL[5::9])
    scope = m.item_scope(items=within)
    ok = scope_ref.mask_of(B0, I0, within=within, exclude=sets)
    full_ids, full_sc = boost_ref.topk(sc_all, ALL, 400, ~ok)
    aid, asc = ref.start(B0)
    for r in range(B0):
        kind = r % 6
        if kind == 1:
            aid[r], asc[r] = full_ids[r, 2], full_sc[r, 2]                      # after entry 3
        elif kind == 2:
            aid[r], asc[r] = full_ids[r, 299], full_sc[r, 299]                  # after entry 300
        elif kind == 3:
            aid[r], asc[r] = -1, -np.inf                                        # exhausted
        elif kind == 4:
            g = sorted(sets[r])[0]                                              # the cursor's item is excluded
            aid[r], asc[r] = g, sc_all[r, g]
        elif kind == 5:
            g = ALL[5::9][r]                                                    # the cursor's item is outside the scope
            aid[r], asc[r] = g, sc_all[r, g]
    for k in (10, 100):
        got = m.recommend(tup, k, exclude="history", within=scope, after=(aid, asc))
        want = ref.page(sc_all, ALL, k, aid, asc, ~ok)
        assert np.array_equal(host(got[0]), want[0]) and _same(host(got[1]), want[1]), k
        assert (host(got[0])[3::6] == -1).all()
        assert np.array_equal(host(got[0])[0::6], full_ids[0::6, :k]) and np.array_equal(host(got[0])[1::6], full_ids[1::6, 3:3 + k])
        # a row's page is its own: the same rows alone, with the cursor as a device holder
        for rows in (slice(0, 1), slice(2, 3), slice(4, 11)):
            few = tuple(x[rows] for x in tup)
            cur = ListCursor(aid[rows], asc[rows], device=m.device)
            assert _equal(m.recommend(few, k, exclude="history", within=scope, after=cur), [t[rows] for t in got]), (k, rows)


# ---- compositions
def test_composes_with_exclusion_scope_category_index_and_boost(base64):
    from tlsan_amd.model import ListCursor
    m, b, cat, tup, sc_all = base64
    sets = history_sets(b)
    within = np.random.RandomState(21).choice(I0, 700, replace=False)
    scope = m.item_scope(items=within)
    c = host(m.last_item_categories(tup)).astype(np.int64)
    c[::7] = -1
    rng = np.random.RandomState(25)
    rows = rng.randint(0, C0, (B0, 3))
    rows[rng.rand(B0, 3) < 0.25] = -1
    rows[[3, 20, 36]] = -1                                                      # rows of negatives only: the unrestricted sub-batch
    idx = m.category_index()
    off, items = lists_ref.index_of(cat, C0)
    ok_idx = lists_ref.union_mask(B0, I0, rows, off, items, exclude=sets)
    ok_idx[(rows < 0).all(1)] = scope_ref.mask_of(B0, I0, exclude=sets)[(rows < 0).all(1)]
    boost = (np.random.RandomState(19).randn(I0) * sc_all.std()).astype(np.float32)
    w = np.random.RandomState(20).randn(B0).astype(np.float32)
    forms = ((dict(), None, sc_all),
             (dict(exclude="history"), scope_ref.mask_of(B0, I0, exclude=sets), sc_all),
             (dict(within=scope), scope_ref.mask_of(B0, I0, within=within), sc_all),
             (dict(category=c), scope_ref.mask_of(B0, I0, category=c, item_cate=cat), sc_all),
             (dict(category=rows, index=idx, exclude="history"), ok_idx, sc_all),
             (dict(boost=boost, boost_weight=w), None, boost_ref.adjusted(sc_all, boost, w)),
             (dict(boost=boost, within=scope, category=c, exclude="history"),
              scope_ref.mask_of(B0, I0, within=within, category=c, item_cate=cat, exclude=sets), boost_ref.adjusted(sc_all, boost)),
             (dict(boost=boost, boost_weight=w, category=rows, index=idx, exclude="history"), ok_idx, boost_ref.adjusted(sc_all, boost, w)))
    for kw, ok, adj in forms:
        for k, pages in ((10, 4), (100, 3)):
            _tiles(m, tup, adj, k, pages, ok=ok, **kw)
        for k in (10, 256):                                                     # no cursor: the call without after=
            assert _equal(m.recommend(tup, k, after=ListCursor.start(B0, m.device), **kw), m.recommend(tup, k, **kw)), (k, kw.keys())


def test_composes_with_a_clustered_index(base64):
    from tlsan_amd.cluster import ClusteredIndex
    from tlsan_amd.model import ListCursor
    m, b, cat, tup, sc_all = base64
    cent = np.random.RandomState(29).randn(8, 64).astype(np.float32)
    ci = ClusteredIndex.from_assignment(ALL % 8, cent, device=m.device, item_b=host(m.item_b))
    boost = (np.random.RandomState(27).randn(I0) * sc_all.std()).astype(np.float32)
    _tiles(m, tup, sc_all, 10, 4, index=ci, probes=8)                           # every list probed: the exact pages
    _tiles(m, tup, boost_ref.adjusted(sc_all, boost), 100, 3, ok=scope_ref.mask_of(B0, I0, exclude=history_sets(b)), index=ci, probes=8,
           boost=boost, exclude="history")
    # fewer probes: every page probes the same lists, so the pages tile the one call of the same probes
    for k, pages in ((10, 5), (64, 4)):
        got = _cat(_walk(m, tup, k, pages, index=ci, probes=3))
        assert _equal(m.recommend(tup, k * pages, index=ci, probes=3), got), k
    assert _equal(m.recommend(tup, 10, index=ci, probes=3, after=ListCursor.start(B0, m.device)), m.recommend(tup, 10, index=ci, probes=3))


# ---- the deep forms
def test_recommend_deep_is_the_chained_pages(base64):
    from tlsan_amd.model import ListCursor
    m, b, cat, tup, sc_all = base64
    sets = history_sets(b)
    ok = scope_ref.mask_of(B0, I0, exclude=sets)
    want = boost_ref.topk(sc_all, ALL, 600, ~ok)
    got = m.recommend_deep(tup, 600, exclude="history")
    assert tuple(got[0].shape) == (B0, 600) and np.array_equal(host(got[0]), want[0]) and _same(host(got[1]), want[1])
    chained = _walk(m, tup, 256, 3, exclude="history")
    assert _equal(got, [x[:, :600] for x in _cat(chained)])
    assert _equal(m.recommend_deep(tup, 600, page=100, exclude="history"), got)             # the page size changes the scans only
    assert _equal(m.recommend_deep(tup, 10, page=100, exclude="history"), m.recommend(tup, 10, exclude="history"))
    # a small scope runs out: the rest is padding; a deep list can start behind a cursor
    few = ALL[::41]
    deep = m.recommend_deep(tup, 300, page=64, within=m.item_scope(items=few))
    want = boost_ref.topk(sc_all, ALL, 300, ~scope_ref.mask_of(B0, I0, within=few))
    assert np.array_equal(host(deep[0]), want[0]) and _same(host(deep[1]), want[1]) and (host(deep[0])[:, len(few):] == -1).all()
    tail = m.recommend_deep(tup, 500, page=256, exclude="history", after=ListCursor.of(got[0][:, :100], got[1][:, :100]))
    assert _equal(tail, [t[:, 100:] for t in got])
    for bad in (dict(diversity=0.3), dict(per_category=2), dict(index=m.shortlist_index())):
        with pytest.raises(ValueError):
            m.recommend_deep(tup, 300, **bad)
        with pytest.raises(ValueError):
            m.recommend(tup, 10, after=ListCursor.start(B0, m.device), **bad)


def test_audience_pages_and_audience_deep(base64):
    from tlsan_amd.model import ListCursor
    m, _, cat, _, _ = base64
    cfg = make_config(U=60, I=I0, C=C0, d=64, H=8)
    b, _ = random_batch(cfg, B=700, Sn=3, seed=71, test=True)
    cuts = ((0, 256), (256, 300), (300, 700))
    parts = [batch_tuple({k: v[lo:hi] for k, v in b.items()}, True) for lo, hi in cuts]
    users = m.user_vectors(parts)
    assert len(users) == 700
    items = np.array([5, 4098, 0, 2048, 5, 1234, 77])                            # a repeated item
    Q = len(items)
    s = np.concatenate([host(m.score_candidates(part, np.tile(items, (len(part[0]), 1)))) for part in parts]).T    # [Q, 700]
    s = np.ascontiguousarray(s)
    want = audience_ref.expected(s, 700)
    rows_all = np.arange(700)
    got = m.audience_deep(items, 600, users)
    assert tuple(got[0].shape) == (Q, 600) and np.array_equal(host(got[0]), want[0][:, :600]) and np.array_equal(bits(host(got[1])), bits(want[1][:, :600]))
    r = host(got[0])
    assert np.array_equal(bits(host(got[1])), bits(s[np.arange(Q)[:, None], r]))    # the score the item has in that user's list
    assert _equal(m.audience_deep(items, 600, users, page=100), got)
    over = m.audience_deep(items, 800, users)                                     # past the rows: padding
    assert np.array_equal(host(over[0])[:, :700], want[0]) and (host(over[0])[:, 700:] == -1).all() and (host(over[1])[:, 700:] == -np.inf).all()
    # pages by hand, against the reference's, with an exclusion list and queries at different depths
    excl = [np.arange(q, 700, 3 + q) for q in range(Q)]
    gone = np.zeros((Q, 700), bool)
    for q in range(Q):
        gone[q, excl[q]] = True
    aid, asc = ref.start(Q)
    aid[1], asc[1] = want[0][1, 299], want[1][1, 299]
    aid[2], asc[2] = -1, -np.inf
    aid[3], asc[3] = excl[3][0], s[3, excl[3][0]]                                # the cursor's row is excluded
    aid[4], asc[4] = 100000, s[4].max()                                          # not a row at all
    for k in (1, 10, 64, 256):
        page = m.audience(items, k, users, exclude=excl, after=(aid, asc))
        wp = ref.page(s, rows_all, k, aid, asc, gone)
        assert np.array_equal(host(page[0]), wp[0]) and np.array_equal(bits(host(page[1])), bits(wp[1])), k
        assert _equal(m.audience(items, k, users, exclude=excl, after=ListCursor.start(Q, m.device)), m.audience(items, k, users, exclude=excl))
    with pytest.raises(ValueError):
        m.audience(items, 10, users, after=ListCursor.start(Q + 1, m.device))

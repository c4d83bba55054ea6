"""List cursors without a GPU: the reference (tests/paging_ref.py) against a brute-force Python sort with the comparison
written out, on tiny rows with NaN, signed zeros, infinities and exact ties and with cursors inside a tie group, at a NaN
entry, at a -inf entry, at an item the row does not hold, at START and exhausted; the reference's own tiling property; the
ABI's three additions (tlsan_eval_topk_scoped_after, tlsan_eval_topk_lists_after, tlsan_dense_topk_after) and their
refusals -- every refusal of the twin with the same code and the new function's name, and a NULL cursor, all before any
launch on fake pointers that are never dereferenced; ListCursor's constructors and argument checks on "cpu"; the argument
errors of recommend / audience / recommend_deep; and the driver's two flags."""
import ctypes as C
import functools
import math
import os
import re
import types

import numpy as np
import pytest

from tests import boost_ref, paging_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_eval_topk_scoped_after", "tlsan_eval_topk_lists_after", "tlsan_dense_topk_after")
NAN, INF = np.float32("nan"), np.float32("inf")


# ---- the reference
def _cmp(a, b):
    """the lists' order as a comparison of (score, id) pairs: negative when a comes first"""
    (sa, ga), (sb, gb) = a, b
    na, nb = math.isnan(sa), math.isnan(sb)
    if na != nb:
        return 1 if na else -1              # NaN after everything else
    if not na and sa != sb:                 # (+0.0 == -0.0 in Python as in IEEE)
        return -1 if sa > sb else 1         # higher first
    return -1 if ga < gb else (1 if ga > gb else 0)


def _brute(row, ids, k, excluded_row, after_id, after_score):
    """one row's page by Python's sort: the eligible entries in order, those the cursor comes strictly before"""
    cand = [(float(s), int(g)) for s, g, x in zip(row, ids, excluded_row) if not x]
    cand.sort(key=functools.cmp_to_key(_cmp))
    if after_id == ref.START:
        return cand[:k]
    if after_id < 0:
        return []
    return [c for c in cand if _cmp((float(after_score), int(after_id)), c) < 0][:k]


def _check_page(adj, ids, k, after_ids, after_scores, excluded=None):
    got_ids, got_sc = ref.page(adj, ids, k, after_ids, after_scores, excluded)
    assert got_ids.dtype == np.int32 and got_sc.dtype == np.float32 and got_ids.shape == (adj.shape[0], k)
    for r in range(adj.shape[0]):
        want = _brute(adj[r], ids, k, np.zeros(len(ids), bool) if excluded is None else excluded[r], int(after_ids[r]), after_scores[r])
        assert got_ids[r, :len(want)].tolist() == [g for _, g in want], (r, after_ids[r], after_scores[r])
        assert np.all(got_ids[r, len(want):] == -1) and np.all(got_sc[r, len(want):] == -np.inf)
        for j, (s, _) in enumerate(want):
            assert (math.isnan(s) and np.isnan(got_sc[r, j])) or got_sc[r, j] == s, (r, j)
            assert not (got_sc[r, j] == 0 and np.signbit(got_sc[r, j]))         # a zero comes back as +0.0
    return got_ids, got_sc


def test_reference_pages_against_a_python_sort():
    # ids                  3     4     5    7     8     9    11    12   20   21    22
    row = np.array([[2.0, 2.0, -0.0, 0.0, -INF, NAN, 2.0, -INF, NAN, INF, 0.25]], np.float32)
    ids = np.array([3, 4, 5, 7, 8, 9, 11, 12, 20, 21, 22])
    full = ref.page(row, ids, 11, *ref.start(1))[0][0].tolist()
    assert full == [21, 3, 4, 11, 22, 5, 7, 8, 12, 9, 20]                        # ties by id, zeros equal, -inf, then NaN
    cursors = [(4, 2.0), (3, 2.0), (11, 2.0),          # inside the tie group of 2.0, at its head and at its end
               (5, 0.0), (5, -0.0), (7, -0.0),         # the zeros' group: the sign of the cursor's zero does not matter
               (9, NAN), (20, NAN), (9, -NAN),         # at a NaN entry, at the last one; the payload / sign does not matter
               (8, -INF), (12, -INF),                  # at a -inf entry
               (6, 2.0), (10, 2.0), (1000, 2.0), (0, 2.0), (6, 1.0), (0, NAN), (15, NAN), (0, INF), (99, -INF),   # not in the row
               (ref.START, 0.0), (ref.START, NAN), (-1, -INF), (-1, 0.0), (-3, 5.0), (-100, NAN)]
    for k in (1, 3, 11, 20):
        for cid, cs in cursors:
            _check_page(row, ids, k, np.array([cid]), np.array([cs], np.float32))
    one = lambda cid, cs, k=11: [g for g in ref.page(row, ids, k, np.array([cid]), np.array([cs], np.float32))[0][0].tolist() if g >= 0]
    assert one(4, 2.0) == [11, 22, 5, 7, 8, 12, 9, 20] and one(6, 2.0) == one(4, 2.0)       # a position, not an item
    assert one(5, 0.0) == one(5, -0.0) == [7, 8, 12, 9, 20]
    assert one(9, NAN) == one(9, -NAN) == [20] and one(20, NAN) == [] and one(0, NAN) == [9, 20]
    assert one(8, -INF) == [12, 9, 20] and one(99, -INF) == [9, 20]
    assert one(ref.START, NAN) == full and one(-1, 0.0) == [] and one(-3, 5.0) == []
    # with exclusions, and several rows at different depths in one call
    rows = np.repeat(row, 4, 0)
    excluded = np.zeros((4, 11), bool)
    excluded[1, [1, 6]] = True
    excluded[2] = True
    got, _ = _check_page(rows, ids, 4, np.array([ref.START, 3, 4, -1]), np.array([0.0, 2.0, 2.0, 0.0], np.float32), excluded)
    assert got.tolist() == [[21, 3, 4, 11], [22, 5, 7, 8], [-1] * 4, [-1] * 4]   # (row 1's cursor item is eligible, 4 and 11 are not)


def test_reference_pages_on_random_rows_and_their_tiling():
    rng = np.random.RandomState(9)
    pool = np.array([NAN, 0.0, -0.0, -INF, INF, 1.5, 1.5, -2.0, 0.25, 0.25, 0.25, 3.0], np.float32)
    for trial in range(30):
        n = int(rng.randint(1, 16))
        ids = np.sort(rng.choice(60, n, replace=False))
        adj = pool[rng.randint(0, len(pool), (3, n))]
        excluded = rng.rand(3, n) < 0.25 if trial % 2 else None
        after_ids = rng.randint(-3, 62, 3)
        after_scores = pool[rng.randint(0, len(pool), 3)]
        for k in (1, 4, 20):
            _check_page(adj, ids, k, after_ids, after_scores, excluded)
        # tiling: the pages chained through their last columns are the whole ranking, then empty pages for ever
        whole_ids, whole_sc = boost_ref.topk(adj, ids, n + 4, excluded)
        for k in (1, 3, 5):
            pages = ref.walk(adj, ids, k, (n + 4 + k - 1) // k + 2, excluded)
            cat_ids = np.concatenate([p[0] for p in pages], 1)
            cat_sc = np.concatenate([p[1] for p in pages], 1)
            assert np.array_equal(cat_ids[:, :n + 4], whole_ids), (trial, k)
            assert np.array_equal(cat_sc[:, :n + 4].view(np.int32), whole_sc.view(np.int32)) or \
                np.all((cat_sc[:, :n + 4] == whole_sc) | (np.isnan(cat_sc[:, :n + 4]) & np.isnan(whole_sc)))
            assert (cat_ids[:, n + 4:] == -1).all() and (cat_sc[:, n + 4:] == -np.inf).all()
            assert (pages[-1][0] == -1).all() and (pages[-2][0] == -1).all()      # exhausted stays exhausted


# ---- the ABI
def test_header_and_exports():
    from tlsan_amd import _lib as L, build
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    lib = L.load()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert re.search(r"const int32_t\*\s+after_ids,\s*const float\*\s+after_scores\s*$", m.group(1)), name
        assert name in L.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+TLSAN_AFTER_START\s+\(-2\)", hdr) and L.AFTER_START == -2 == ref.START
    assert "tlsan_after.hip" in build.SOURCES
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)             # additions: the version stays
    assert L.ABI_VERSION == 15 and lib.tlsan_abi_version() == 15


def test_arguments_are_refused_without_a_launch():
    from tlsan_amd import _lib as L
    lib = L.load()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    bad_dims = L.Dims(100, 200, 10, 128, 64, 32, 8, 10)       # d_item + d_cate != d
    unsupported = L.Dims(100, 200, 10, 96, 48, 48, 8, 10)     # d = 96
    fake = 0x1000                       # never dereferenced: every call below is refused by the argument checks
    p = L.Params(*([fake] * 8))
    hole = L.Params(*([fake] * 8))
    hole.item_cate = None
    err = lambda: lib.tlsan_last_error()
    ref_of = lambda d: C.byref(d) if d else None

    def scoped(after, d=dims, pp=p, ut=fake, B=4, K=16, off=None, xid=None, sub=fake, nsub=50, cate=fake, mul=1, add=0, ids=fake,
               scores=fake, ws=fake, ws_bytes=1 << 40, boost=fake, weight=None, aid=fake, asc=fake):
        args = (ref_of(d), ref_of(pp), ut, B, K, off, xid, sub, nsub, cate, mul, add, ids, scores, ws, C.c_size_t(ws_bytes), None)
        if after:
            return lib.tlsan_eval_topk_scoped_after(*args, boost, weight, aid, asc)
        return lib.tlsan_eval_topk_scoped_boost(*args, boost, weight) if boost else lib.tlsan_eval_topk_scoped(*args)

    def lists(after, d=dims, pp=p, ut=fake, B=4, K=16, off=None, xid=None, loff=fake, items=fake, nl=10, ml=50, rows=fake, P=2,
              mul=1, add=0, ids=fake, scores=fake, ws=fake, ws_bytes=1 << 40, boost=fake, weight=None, aid=fake, asc=fake):
        args = (ref_of(d), ref_of(pp), ut, B, K, off, xid, loff, items, nl, ml, rows, P, mul, add, ids, scores, ws,
                C.c_size_t(ws_bytes), None)
        if after:
            return lib.tlsan_eval_topk_lists_after(*args, boost, weight, aid, asc)
        return lib.tlsan_eval_topk_lists_boost(*args, boost, weight) if boost else lib.tlsan_eval_topk_lists(*args)

    def dense(after, q=fake, Q=4, d=128, x=fake, N=1000, scale=None, bias=None, off=None, xid=None, add=0, K=16, ids=fake, scores=fake,
              ws=fake, ws_bytes=1 << 40, aid=fake, asc=fake, boost=None, weight=None):
        args = (q, Q, d, x, N, scale, bias, off, xid, add, K, ids, scores, ws, C.c_size_t(ws_bytes), None)
        return lib.tlsan_dense_topk_after(*args, aid, asc) if after else lib.tlsan_dense_topk(*args)

    need_s = lib.tlsan_scope_workspace_bytes(C.byref(dims), 4, 16, 50)
    need_l = lib.tlsan_lists_workspace_bytes(C.byref(dims), 4, 2, 16, 10, 50)
    need_d = lib.tlsan_dense_topk_workspace_bytes(4, 1000, 16)
    assert need_s > 0 and need_l > 0 and need_d > 0
    shared = (dict(ids=None), dict(scores=None), dict(ut=None), dict(B=0), dict(B=-2), dict(K=0), dict(K=257), dict(K=-1),
              dict(d=None), dict(d=bad_dims), dict(d=unsupported), dict(pp=None), dict(pp=hole), dict(off=fake), dict(xid=fake),
              dict(mul=0), dict(add=-1), dict(mul=1 << 30), dict(ws=None), dict(ws_bytes=0))
    scoped_only = (dict(sub=None, nsub=0), dict(sub=None, nsub=7), dict(sub=fake, nsub=-1), dict(nsub=201), dict(sub=None, nsub=201),
                   dict(ws_bytes=need_s - 1), dict(sub=None, nsub=-1, ws_bytes=0))
    lists_only = (dict(P=0), dict(P=9), dict(P=-1), dict(nl=0), dict(nl=-3), dict(nl=(1 << 24) + 1), dict(B=(1 << 24) + 1),
                  dict(ml=-1), dict(loff=None), dict(items=None), dict(rows=None), dict(ws_bytes=need_l - 1))
    dense_cases = (dict(q=None), dict(x=None), dict(ids=None), dict(scores=None), dict(off=fake), dict(xid=fake), dict(d=96), dict(d=0),
                   dict(Q=0), dict(Q=(1 << 24) + 1), dict(N=0), dict(N=(1 << 30) + 1), dict(K=0), dict(K=257), dict(add=-1),
                   dict(add=(1 << 31) - 10), dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=need_d - 1))
    n = 0
    for fn, name, cases, boosts in ((scoped, NAMES[0], shared + scoped_only, (fake, None)), (lists, NAMES[1], shared + lists_only, (fake, None)),
                                    (dense, NAMES[2], dense_cases, (None,))):
        for kw in cases:
            for boost in boosts:                                                 # the twin: the boosted call, or the plain one
                for weight in ((None, fake) if boost else (None,)):
                    twin = fn(False, boost=boost, weight=weight, **kw)
                    assert twin in (-1, -2, -4), (name, kw, twin)                # BADARG, WORKSPACE, UNSUPPORTED: refused
                    assert fn(True, boost=boost, weight=weight, **kw) == twin, (name, kw)      # the same code ...
                    assert name.encode() in err(), (name, kw, err())                         # ... under the new function's name
                    n += 1
        for kw in (dict(aid=None), dict(asc=None), dict(aid=None, asc=None)):
            assert fn(True, **kw) == -1 and name.encode() in err() and b"without a cursor" in err(), (name, kw, err())
            n += 1
    assert b"tlsan_dense_topk is the call" in err()
    assert scoped(True, aid=None) == -1 and b"tlsan_eval_topk_scoped_boost is the call" in err()
    assert scoped(True, aid=None, boost=None) == -1 and b"tlsan_eval_topk_scoped is the call" in err()
    assert lists(True, asc=None, boost=None) == -1 and b"tlsan_eval_topk_lists is the call" in err()
    assert scoped(True, aid=None, ws_bytes=0) == -1                              # (a NULL cursor is refused ahead of the workspace)
    for fn, name in ((scoped, NAMES[0]), (lists, NAMES[1])):                     # a weight weighs a boost
        assert fn(True, boost=None, weight=fake) == -1 and name.encode() in err() and b"row_weight" in err()
    assert n > 150


# ---- ListCursor
def test_list_cursor_construction_and_checks():
    import torch
    from tlsan_amd.model import ListCursor, cursor_of, check_deep
    c = ListCursor([5, -1, -2], [1.5, float("-inf"), 0], device="cpu")
    assert c.ids.dtype == torch.int32 and c.scores.dtype == torch.float32 and len(c) == 3
    assert c.ids.tolist() == [5, -1, -2] and c.done.tolist() == [False, True, False] and c.done.dtype == torch.bool
    assert ListCursor.START == -2
    s = ListCursor.start(4, "cpu")
    assert s.ids.tolist() == [-2] * 4 and s.scores.tolist() == [0.0] * 4 and not s.done.any()
    ids = torch.tensor([[3, 9, 4], [7, -1, -1]], dtype=torch.int32)
    sc = torch.tensor([[2.0, 1.0, float("nan")], [0.5, float("-inf"), float("-inf")]])
    o = ListCursor.of(ids, sc)
    assert o.ids.tolist() == [4, -1] and torch.isnan(o.scores[0]) and o.scores[1] == float("-inf") and o.done.tolist() == [False, True]
    ids[0, 2] = 77                                                              # cloned: the page may be overwritten
    assert o.ids.tolist() == [4, -1] and o.ids.is_contiguous()
    assert ListCursor(np.array([1, 2], np.int64), np.array([1, 2], np.int64)).scores.tolist() == [1.0, 2.0]
    assert ListCursor(torch.tensor([1]), torch.tensor([0.5], dtype=torch.float64)).scores.dtype == torch.float32
    assert c.rows(torch.tensor([2, 0])).ids.tolist() == [-2, 5]
    for bad in (([1.5], [1.0]), ([[1]], [[1.0]]), ([], []), ([1, 2], [1.0]), (np.zeros(2, bool), [0.0, 0.0]), ([1], [1j]), ([1 << 40], [0.0]), (3, 1.0)):
        with pytest.raises(ValueError):
            ListCursor(*bad)
    for bad in ((ids[0], sc[0]), (ids, sc[:, :2]), (ids.numpy(), sc.numpy()), (ids[:, :0], sc[:, :0])):
        with pytest.raises(ValueError):
            ListCursor.of(*bad)
    with pytest.raises(ValueError):
        ListCursor.start(0)
    # after= as the calls check it
    assert cursor_of(None, 3, "cpu") is None
    assert cursor_of(c, 3, "cpu").ids.data_ptr() == c.ids.data_ptr()            # a holder is reused, not copied
    w = cursor_of((np.array([4, 5, 6]), [0.5, 0.25, 1]), 3, "cpu")
    assert isinstance(w, ListCursor) and w.ids.tolist() == [4, 5, 6] and w.scores.tolist() == [0.5, 0.25, 1.0]
    for bad, B in ((c, 4), (c, 2), (([1, 2], [1.0, 2.0]), 3), (([1, 2], [1.0]), 2), (([1.0, 2.0], [1.0, 2.0]), 2), ([1, 2], 2), ("start", 2),
                   (([1, 2], [1.0, 2.0], [0, 0]), 2), ((["a", "b"], [1.0, 2.0]), 2)):
        with pytest.raises(ValueError):
            cursor_of(bad, B, "cpu")
    assert check_deep(600, 256) == (600, 256) and check_deep(np.int64(1), 1) == (1, 1)
    for n, page in ((0, 256), (-5, 10), (10, 0), (10, 257), (10.0, 10), (10, True), ("10", 10)):
        with pytest.raises(ValueError):
            check_deep(n, page)


def test_deep_pages_chain_the_cursors():
    """deep_pages on the reference: the pages asked for, the last one short, every cursor the column before"""
    import torch
    from tlsan_amd.model import deep_pages
    rng = np.random.RandomState(3)
    adj = rng.randint(-3, 4, (5, 40)).astype(np.float32)                         # many ties
    adj[0, :30] = np.nan
    ids = np.arange(40) * 3
    asked = []

    def topk(k, after):
        asked.append((k, after))
        a = ref.start(5) if after is None else (after.ids.numpy(), after.scores.numpy())
        return tuple(torch.as_tensor(x) for x in ref.page(adj, ids, k, a[0], a[1]))
    for n, page in ((40, 7), (55, 16), (7, 7), (5, 256), (15, 5)):
        del asked[:]
        got_ids, got_sc = deep_pages(topk, n, page)
        want_ids, want_sc = boost_ref.topk(adj, ids, n)
        assert np.array_equal(got_ids.numpy(), want_ids) and got_sc.shape == (5, n)
        assert np.array_equal(np.nan_to_num(got_sc.numpy(), nan=7e7), np.nan_to_num(want_sc, nan=7e7))
        assert [k for k, _ in asked] == [page] * (n // page) + ([n % page] if n % page else [])
        assert asked[0][1] is None and all(a is not None for _, a in asked[1:])


# ---- the models' argument checks (before any launch: no device is touched)
def test_recommend_and_audience_argument_errors():
    from tlsan_amd.dist import ShardedModel
    from tlsan_amd.model import Model
    from tlsan_amd.shortlist import ShortlistIndex
    batch = tuple(np.zeros(6, np.int32) for _ in range(4))                       # six rows; never looked at

    def stub(cls):
        """what the checks look at of a model, with the class's own shared steps bound to it"""
        me = types.SimpleNamespace(device="cpu", config=dict(item_count=50, cate_count=5, hidden_units=64), I=50, C=5)
        me._recommend_lists = functools.partial(cls._recommend_lists, me)
        me._audience_lists = functools.partial(cls._audience_lists, me)
        return me
    cur = (np.arange(6), np.zeros(6, np.float32))
    short = ShortlistIndex.__new__(ShortlistIndex)
    for cls in (Model, ShardedModel):
        for kw in (dict(after=(np.arange(5), np.zeros(5, np.float32))), dict(after=(np.arange(7), np.zeros(7, np.float32))),
                   dict(after=(np.zeros(6, np.float32), np.zeros(6, np.float32))), dict(after=np.arange(6)), dict(after="start")):
            with pytest.raises(ValueError, match="after|ListCursor"):
                cls.recommend(stub(cls), batch, 5, **kw)
            with pytest.raises(ValueError, match="after|ListCursor"):
                cls.recommend_deep(stub(cls), batch, 20, page=5, **kw)
    for kw in (dict(diversity=0.3), dict(per_category=2), dict(per_category=1, pool=32), dict(diversity=0.5, per_category=2)):
        with pytest.raises(ValueError, match="second stage"):
            Model._recommend_lists(stub(Model), batch, 5, True, **kw)
        for cls in (Model, ShardedModel):
            with pytest.raises(ValueError, match="second stage"):
                cls.recommend_deep(stub(cls), batch, 20, page=5, **kw)
            with pytest.raises(ValueError, match="second stage"):
                cls.recommend(stub(cls), batch, 5, after=cur, **kw)
    with pytest.raises(ValueError, match="ShortlistIndex"):
        Model.recommend(stub(Model), batch, 5, after=cur, index=short)
    with pytest.raises(ValueError, match="ShortlistIndex"):
        Model.recommend_deep(stub(Model), batch, 20, page=5, index=short)
    for n, page in ((0, 5), (20, 0), (20, 257), (2.5, 5)):
        for cls in (Model, ShardedModel):
            with pytest.raises(ValueError):
                cls.recommend_deep(stub(cls), batch, n, page=page)
            with pytest.raises(ValueError):
                cls.audience_deep(stub(cls), [1, 2], n, None, page=page)
    # audience: the items are checked, then the cursor's length against them
    for cls in (Model, ShardedModel):
        for after in ((np.arange(3), np.zeros(3, np.float32)), (np.arange(1), np.zeros(1, np.float32)), "x"):
            with pytest.raises(ValueError, match="after|ListCursor"):
                cls.audience(stub(cls), [1, 2], 5, None, after=after)
        with pytest.raises(ValueError, match="items"):
            cls.audience(stub(cls), [1, 50], 5, None, after=(np.arange(2), np.zeros(2, np.float32)))


# ---- the driver
def test_driver_flags():
    from tlsan_amd import train as T
    args = T.parse(["--dataset", "x.npz"])
    assert args.recommend_pages == 1 and args.audience_pages == 1
    args = T.parse(["--dataset", "x.npz", "--recommend_k", "20", "--recommend_pages", "30", "--recommend_exclude", "history"])
    assert args.recommend_k == 20 and args.recommend_pages == 30
    args = T.parse(["--dataset", "x.npz", "--audience_k", "256", "--audience_pages", "16", "--audience_items", "3,7"])
    assert args.audience_k == 256 and args.audience_pages == 16
    T.parse(["--dataset", "x.npz", "--recommend_k", "20", "--recommend_pages", "1", "--recommend_metrics", "1"])    # one page: as ever
    for bad in (["--recommend_pages", "3"], ["--audience_pages", "2"], ["--recommend_k", "5", "--recommend_pages", "0"],
                ["--audience_k", "5", "--audience_items", "1", "--audience_pages", "-1"],
                ["--recommend_k", "5", "--recommend_pages", "2", "--recommend_diversity", "0.3"],
                ["--recommend_k", "5", "--recommend_pages", "2", "--recommend_per_category", "2"],
                ["--recommend_k", "5", "--recommend_pages", "2", "--recommend_per_category", "2", "--recommend_pool", "32"],
                ["--recommend_k", "5", "--recommend_pages", "2", "--shortlist_index", "1"],
                ["--recommend_k", "5", "--recommend_pages", "2", "--recommend_metrics", "1"],
                ["--recommend_k", "5", "--recommend_pages", "2", "--recommend_explain", "3"],
                ["--audience_k", "257", "--audience_pages", "2", "--audience_items", "1"]):
        with pytest.raises(SystemExit):
            T.parse(["--dataset", "x.npz"] + bad)
    assert T.recommend_path("m", 600).endswith("recommend_top600.npz")

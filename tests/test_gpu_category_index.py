"""GPU tests of the per-category item index (CategoryIndex; tlsan_eval_topk_lists / tlsan_similar_topk_lists; recommend's and
similar_items' index=): the indexed lists equal the category form without an index bit for bit, and equal the selection of
tests/scope_ref.py from the model's own scores (score_candidates) over the union of the probed lists (tests/lists_ref.py);
ties and NaN, independence of the batch, of the row order and of the grouping, the scope inside the index, the diversified
form, similar_items, a hostile index through the raw entry, the state, and the driver's flag.

The table: 1 200 items in 9 categories of 0, 1, 15, 16, 17, 255, 257, 600 and 39 items (the 600 make three slices of the
37-row launch, so the shorter lists have slices that start past their end).  37 rows ask, in the [B] form, for one list 17
times (two groups), one 16 times, one once, and the three rows that 17 + 16 + 1 leave for the empty list and for nothing (-1), under two
such assignments; the [B, P] cases have several unrestricted rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lists_ref, scope_ref as ref
from tests.helpers import (batch_tuple, bits, history_sets, host, lazy_model, make_config, model, p32, random_batch,
                           random_params)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 15, 16, 17, 255, 257, 600, 39)
I0, C0, B0 = sum(SIZES), len(SIZES), 37
CAT = np.random.RandomState(5).permutation(np.repeat(np.arange(C0), SIZES)).astype(np.int32)
ASKS = (np.array([7] * 17 + [5] * 16 + [1] + [0, 0] + [-1]), np.array([3] + [-1] + [6] * 17 + [0] + [4] * 16 + [2]))
assert all(len(c) == B0 for c in ASKS)
KS = (1, 10, 64)


def _same(a, b):
    """float32 arrays equal in bits, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _equal(a, b):
    a, b = [host(t) for t in a], [host(t) for t in b]
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1])


def _case(d=64, H=8, **kw):
    cfg = make_config(U=60, I=I0, C=C0, d=d, H=H)
    p = p32(random_params(cfg, seed=31))
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=32, test=True)
    m = model(cfg, CAT, p, **kw)
    tup = batch_tuple(b, True)
    return m, b, tup, host(m.score_candidates(tup, np.tile(np.arange(I0), (B0, 1))))


@pytest.fixture(scope="module")
def base64():
    m, b, tup, sc_all = _case()
    return m, b, tup, sc_all, m.category_index()


def _wipe():
    """an explicit exclusion list that removes two small lists whole"""
    return [np.nonzero((CAT == 1) | (CAT == 2))[0]] * B0


# ---- 1. the category form, bit for bit, and the reference's selection from the model's own scores
@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (128, 4)])
def test_indexed_lists_equal_the_category_form_and_the_reference(d, H):
    m, b, tup, sc_all = _case(d, H)
    idx = m.category_index()
    assert idx.max_list == 600 and host(idx.list_off).tolist() == np.concatenate([[0], np.cumsum(SIZES)]).tolist()
    for c in ASKS:
        for exclude, sets in ((None, None), ("history", history_sets(b)), (_wipe(), _wipe())):
            ok = ref.mask_of(B0, I0, category=c, item_cate=CAT, exclude=sets)
            for k in KS:
                got = m.recommend(tup, k, exclude=exclude, category=c, index=idx)
                assert _equal(got, m.recommend(tup, k, exclude=exclude, category=c)), (k, type(exclude))
                ids, sc = (host(t) for t in got)
                want_ids, want_sc = ref.topk(sc_all, ok, k)
                assert ids.dtype == np.int32 and np.array_equal(ids, want_ids), (k, type(exclude))
                assert _same(sc, want_sc), (k, type(exclude))
            assert (ids[c == 0] == -1).all() and (sc[c == 0] == -np.inf).all()          # the empty list
            assert (ids[(c >= 0) & (np.asarray(SIZES)[c] < 64), -1] == -1).all()         # K = 64 exceeds several lists
            assert (ids[c < 0] >= 0).all()                                               # the unrestricted rows are full


@pytest.mark.parametrize("table_dtype", ["bf16", "f32"])
def test_lazy_l2_and_bf16_tables(table_dtype):
    cfg, m = lazy_model(1000, table_dtype, seed=41)            # d = 256, 31 categories, P != 1
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=43, test=True)
    tup = batch_tuple(b, True)
    idx = m.category_index()
    c = host(m.last_item_categories(tup)).astype(np.int64)
    c[::9] = -1
    sc_all = host(m.score_candidates(tup, np.tile(np.arange(1000), (B0, 1))))
    cat = host(m.item_cate)
    for exclude, sets in ((None, None), ("history", history_sets(b))):
        for k in KS:
            got = m.recommend(tup, k, exclude=exclude, category=c, index=idx)
            assert _equal(got, m.recommend(tup, k, exclude=exclude, category=c)), (k, exclude)
            want_ids, want_sc = ref.topk(sc_all, ref.mask_of(B0, 1000, category=c, item_cate=cat, exclude=sets), k)
            assert np.array_equal(host(got[0]), want_ids) and _same(host(got[1]), want_sc), (k, exclude)


# ---- 2. the [B, P] form: the union of the probed lists
def _probes():
    rng = np.random.RandomState(11)
    rows = rng.randint(0, C0, (B0, 3))
    rows[:, 1] = np.where(rng.rand(B0) < 0.4, rows[:, 0], rows[:, 1])          # a repeated id counts once
    rows[rng.rand(B0, 3) < 0.25] = -1
    rows[[3, 20, 36]] = -1                                                      # unrestricted rows
    rows[5] = [7, 7, 7]
    rows[6] = [0, -1, 0]                                                        # the empty list alone
    rows[7] = [-1, -1, 2]
    return rows


def test_union_of_probed_lists(base64):
    m, b, tup, sc_all, idx = base64
    rows = _probes()
    assert (rows[:, 0] == rows[:, 1]).sum() > 5 and ((rows < 0).all(1)).sum() >= 3
    off, items = lists_ref.index_of(CAT, C0)
    free = (rows < 0).all(1)
    for exclude, sets in ((None, None), ("history", history_sets(b))):
        ok = lists_ref.union_mask(B0, I0, rows, off, items, exclude=sets)
        ok[free] = ref.mask_of(B0, I0, exclude=sets)[free]
        for k in KS:
            ids, sc = (host(t) for t in m.recommend(tup, k, exclude=exclude, category=rows, index=idx))
            want_ids, want_sc = ref.topk(sc_all, ok, k)
            assert np.array_equal(ids, want_ids) and _same(sc, want_sc), (k, exclude)
    for c in ASKS:                                                              # [B, 1] is [B]
        assert _equal(m.recommend(tup, 10, category=c[:, None], index=idx), m.recommend(tup, 10, category=c, index=idx))
    # every list at once: the whole table
    everything = np.tile(np.arange(8), (B0, 1))
    got = m.recommend(tup, 64, category=np.concatenate([everything[:, :7], np.full((B0, 1), 8)], 1), index=idx)
    want = ref.topk(sc_all, np.asarray(CAT != 7)[None, :].repeat(B0, 0), 64)
    assert np.array_equal(host(got[0]), want[0]) and _same(host(got[1]), want[1])


# ---- 3. ties and NaN
def test_ties_and_nan_inside_a_list():
    cfg = make_config(U=60, I=I0, C=C0, d=64)
    p = p32(random_params(cfg, seed=71))
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=72, test=True)
    in5 = np.nonzero(CAT == 5)[0]
    tied = in5[10:50:2]                             # 20 items of one list: bit-identical rows, far ahead of the rest
    p["item_emb"][tied] = p["item_emb"][tied[0]]
    p["item_b"][tied] = 1000.0
    nan_item = int(in5[100])
    p["item_b"][nan_item] = np.nan
    for k in ("i", "j", "hist_i", "hist_i_new"):
        b[k] = np.where(b[k] == nan_item, nan_item + 1, b[k])
    m = model(cfg, CAT, p)
    tup = batch_tuple(b, True)
    idx = m.category_index()
    c = np.full(B0, 5)
    ids, sc = (host(t) for t in m.recommend(tup, 12, category=c, index=idx))
    assert np.all(ids == tied[:12][None, :]) and np.all(sc == sc[:, :1])        # equal scores: the lower id first
    assert _equal(m.recommend(tup, 12, category=c, index=idx), m.recommend(tup, 12, category=c))
    full = m.recommend(tup, 256, category=c, index=idx)
    assert _equal(full, m.recommend(tup, 256, category=c))
    ids, sc = (host(t) for t in full)
    assert np.all(ids[:, 254] == nan_item) and np.all(np.isnan(sc[:, 254]))     # the NaN comes last, before the padding
    assert np.all(ids[:, 255] == -1) and np.all(sc[:, 255] == -np.inf) and np.all(np.isfinite(sc[:, :254]))


# ---- 4. a row's result depends on its own inputs only
def test_independence_of_order_batch_and_grouping(base64):
    m, b, tup, _, idx = base64
    rows = _probes()
    perm = np.random.RandomState(3).permutation(B0)
    for c in (ASKS[0], rows):
        for exclude in (None, "history"):
            base = [host(t) for t in m.recommend(tup, 10, exclude=exclude, category=c, index=idx)]
            again = [host(t) for t in m.recommend(tup, 10, exclude=exclude, category=c, index=idx)]      # the grouping's freedom
            assert np.array_equal(base[0], again[0]) and _same(base[1], again[1])
            shuffled = batch_tuple({k: v[perm] for k, v in b.items()}, True)
            got = [host(t) for t in m.recommend(shuffled, 10, exclude=exclude, category=c[perm], index=idx)]
            assert np.array_equal(got[0], base[0][perm]) and _same(got[1], base[1][perm])
            for r in (0, 16, 17, 33, 35):                                       # alone: B = 1
                one = batch_tuple({k: v[r:r + 1] for k, v in b.items()}, True)
                got = [host(t) for t in m.recommend(one, 10, exclude=exclude, category=c[r:r + 1], index=idx)]
                assert np.array_equal(got[0], base[0][r:r + 1]) and _same(got[1], base[1][r:r + 1]), r


# ---- 5. the scope inside the index; the diversified form
def test_index_over_a_scope_and_diversified(base64):
    m, b, tup, _, idx = base64
    scope = m.item_scope(items=np.arange(0, I0, 3))
    sidx = m.category_index(within=scope)
    assert sidx.count == scope.count and sidx.max_list == int((CAT[::3] == 7).sum())
    for c in ASKS:
        for k in KS:
            for exclude in (None, "history"):
                assert _equal(m.recommend(tup, k, exclude=exclude, category=c, index=sidx),
                              m.recommend(tup, k, exclude=exclude, category=c, within=scope)), (k, exclude)
        for kw in (dict(diversity=0.3, pool=64), dict(per_category=2, diversity=0.5), dict(per_category=1, pool=32, exclude="history")):
            assert _equal(m.recommend(tup, 10, category=c, index=idx, **kw), m.recommend(tup, 10, category=c, **kw)), list(kw)
            assert _equal(m.recommend(tup, 10, category=c, index=sidx, **kw), m.recommend(tup, 10, category=c, within=scope, **kw))
    empty = m.category_index(within=m.item_scope(items=[]))
    ids, sc = (host(t) for t in m.recommend(tup, 5, category=ASKS[0], index=empty))
    assert np.all(ids == -1) and np.all(sc == -np.inf)         # (the unrestricted row too: the scope is the index's)


# ---- 6. similar_items
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_similar_items_with_an_index(base64, metric):
    m, _, _, _, idx = base64
    qids = np.concatenate([np.arange(0, I0, 29), [np.nonzero(CAT == c)[0][0] for c in range(1, C0)], [I0 - 1]])
    excl = [[int(q) // 2, 3, 6, 9] + np.nonzero(CAT == 2)[0][:5].tolist() for q in qids]
    for exclude in (None, excl):
        for k in (5, 64):
            got = m.similar_items(qids, k, metric=metric, exclude=exclude, same_category=True, index=idx)
            assert _equal(got, m.similar_items(qids, k, metric=metric, exclude=exclude, same_category=True)), (k, exclude is None)
            ids = host(got[0])
            assert not np.any(ids == qids[:, None])                             # the query is never in its own list
            assert np.all(np.where(ids >= 0, CAT[np.maximum(ids, 0)], CAT[qids][:, None]) == CAT[qids][:, None])
    assert np.all(host(m.similar_items([int(np.nonzero(CAT == 1)[0][0])], 3, metric=metric, same_category=True, index=idx)[0]) == -1)


# ---- 7. a hostile index through the raw entry
def test_hostile_index_entries_are_never_selected(base64):
    import torch
    from tlsan_amd import model as M
    m, _, tup, sc_all, _ = base64
    listed = np.array([-1, 0, 5, I0 + 5, 6, 300, I0 - 1, -1, 7, 8, I0 + 5, 9])          # lists 0, 1, 2 of 4 / 5 / 3 entries; 3 empty
    off = np.array([0, 4, 9, 12, 12])
    lists = (torch.as_tensor(off.astype(np.int32)).to(m.device), torch.as_tensor(listed.astype(np.int32)).to(m.device), 5)
    rows = np.tile(np.array([[0, 1], [4 + 3, 2], [1, 4 + 3], [3, -1], [2, 0]]), (8, 1))[:B0]   # nlists + 3: no probe
    ok = lists_ref.union_mask(B0, I0, rows, off, listed)
    assert ok.sum(1).tolist()[:5] == [6, 2, 4, 0, 4]
    _, _, ut, db = m.forward(tup, is_test=True, want_u_t=True)
    rl = torch.as_tensor(rows.astype(np.int32)).to(m.device).contiguous()
    for k in (1, 3, 10):
        ids, sc = (host(t) for t in M.lists_topk(m.lib, m.dims, m.cparams, ut, db.B, k, (None, None), lists, rl, 1, 0,
                                                 m._topk_workspace, m._stream()))      # (L.check: the call returned 0)
        want_ids, want_sc = ref.topk(sc_all, ok, k)
        assert np.array_equal(ids, want_ids) and _same(sc, want_sc), k


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
    idx = m.category_index()
    c = m.last_item_categories(tup)
    m.recommend(tup, 5, category=c, index=idx)                   # (what the last step owed lands with the first call)
    P = m.table_scale()
    assert P != 1.0
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.cate_emb, m.item_b, m.dense)]
    before = snap()
    m.recommend(tup, 20, category=c, index=idx, exclude="history")
    m.recommend(tup, 5, category=np.tile(np.arange(3), (30, 1)), index=idx, per_category=1, diversity=0.5)
    m.similar_items(np.arange(0, 500, 23), 10, same_category=True, index=idx)
    m.similar_items(np.arange(0, 500, 23), 10, metric="dot", same_category=True, index=idx)
    after = snap()
    assert m.table_scale() == P
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, after))
    other = model(make_config(U=40, I=400, C=7, d=128, H=8), cat[:400]).category_index()
    for kw in (dict(index=idx), dict(index=other, category=c), dict(index=idx, category=np.full(30, 7)),
               dict(index=idx, category=np.zeros((30, 9), np.int64)), dict(index=idx, category=np.zeros(29, np.int64)),
               dict(index=idx, category=c, within=m.item_scope(items=[1])), dict(index=[1, 2], category=c)):
        with pytest.raises(ValueError):
            m.recommend(tup, 5, **kw)
    for kw in (dict(index=idx), dict(index=other, same_category=True), dict(index=idx, same_category=True, within=m.item_scope(items=[1]))):
        with pytest.raises(ValueError):
            m.similar_items([1, 2], 5, **kw)
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, snap()))


# ---- 9. the driver
@pytest.mark.parametrize("flags", [("--recommend_same_category", "1", "--similar_k", "5", "--similar_same_category", "1"),
                                   ("--recommend_categories", "3,7,12", "--recommend_same_category", "1")])
def test_driver_writes_the_same_files_with_the_index(tmp_path, flags):
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    files = []
    for on in ("0", "1"):
        out = str(tmp_path / ("model" + on))
        r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "30",
                            "--eval_freq", "1000", "--quiet", "--recommend_k", "10", "--recommend_exclude", "none",
                            "--category_index", on] + list(flags), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        files.append({n: np.load(os.path.join(out, n)) for n in sorted(os.listdir(out)) if n.endswith(".npz") and
                      (n.startswith("recommend_top") or n.startswith("similar-"))})
    assert list(files[0]) == list(files[1]) and "recommend_top10.npz" in files[0]
    assert ("similar-5.npz" in files[0]) == ("--similar_k" in flags)
    for n in files[0]:
        assert sorted(files[0][n].files) == sorted(files[1][n].files)
        for key in files[0][n].files:               # (an .npz carries its members' time stamps: the arrays are what is written)
            a, z = files[0][n][key], files[1][n][key]
            assert a.dtype == z.dtype and a.shape == z.shape and a.tobytes() == z.tobytes(), (n, key)

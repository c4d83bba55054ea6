"""GPU tests of the category shelves (Model.shelves; tlsan_eval_shelves): a row's page equals the per-category calls
recommend(category=full(c), index=idx) shelf by shelf, ids and score bits, and the numpy reference (tests/shelves_ref.py) on
the model's own scores (score_candidates); independence of the scan's plan, of the batch, the row order and a repeated
call; ties and NaN; min_items and rank_at; skip; the scope inside the index; a hostile index through the raw helper; lazy
L2 and bf16 tables; the state; list_metrics on a flattened page; the driver's flags.

Table A is test_gpu_category_index.py's: 1 200 items in 9 categories of 0, 1, 15, 16, 17, 255, 257, 600 and 39 items, 37
rows.  Table B: 1 500 items in 45 categories -- three empty, four of one item, 15, 16, 17, 255, 257, 600 and 32 of 3 to 18
items -- so that there are more categories with items (42) than any S, at least three segments at seg_items=300 and two
big lists (one of two slices, one of three) at big_items=256."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lists_ref, scope_ref, shelves_ref as ref
from tests.helpers import (batch_tuple, bits, history_sets, host, lazy_model, make_config, model, p32, random_batch,
                           random_params)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B0 = 37
SIZES_A = (0, 1, 15, 16, 17, 255, 257, 600, 39)
_FILL = [3 + (7 * i) % 16 for i in range(32)]
SIZES_B = (0, 1, 15, 255) + tuple(_FILL[:10]) + (0, 1, 16, 600) + tuple(_FILL[10:20]) + (1, 17, 257, 0) + tuple(_FILL[20:]) + (1,)
assert len(SIZES_B) == 45 and SIZES_B.count(0) == 3 and SIZES_B.count(1) == 4 and 1450 <= sum(SIZES_B) <= 1550
TABLES = {"A": SIZES_A, "B": SIZES_B}
CATS = {t: np.random.RandomState(5 + len(s)).permutation(np.repeat(np.arange(len(s)), s)).astype(np.int32) for t, s in TABLES.items()}
WIPED = {"A": (1, 2), "B": (1, 2)}          # two small categories (1 and 15 items in both tables) an exclusion list removes whole
PAGES = ((1, 1), (3, 10), (9, 10), (4, 64), (32, 8))
PLANS = (dict(), dict(seg_items=300, big_items=256), dict(seg_items=64, big_items=16), dict(seg_items=256, big_items=0))


def _same(a, b):
    """float32 arrays equal in bits, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _equal(a, b):
    """pages (cats, ids, scores) or lists (ids, scores) equal: integers exactly, scores in bits"""
    a, b = [np.asarray(t) if isinstance(t, np.ndarray) else host(t) for t in a], [np.asarray(t) if isinstance(t, np.ndarray) else host(t) for t in b]
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a[:-1], b[:-1])) and _same(a[-1], b[-1])


class Case:
    def __init__(self, table="A", d=64, H=8, seed=31, edit=None, **kw):
        self.cat = CATS[table]
        self.I, self.C = len(self.cat), len(TABLES[table])
        self.cfg = make_config(U=60, I=self.I, C=self.C, d=d, H=H)
        p = p32(random_params(self.cfg, seed=seed))
        self.b, _ = random_batch(self.cfg, B=B0, Sn=3, seed=seed + 1, test=True)
        if edit is not None:
            edit(p, self.b)
        self.m = model(self.cfg, self.cat, p, **kw)
        self.tup = batch_tuple(self.b, True)
        self.sc_all = host(self.m.score_candidates(self.tup, np.tile(np.arange(self.I), (B0, 1))))
        self.idx = self.m.category_index()
        self.off, self.items = lists_ref.index_of(self.cat, self.C)

    def mask(self, exclude=None, within=None):
        return scope_ref.mask_of(B0, self.I, exclude=exclude, within=within)


@pytest.fixture(scope="module")
def case_a():
    return Case("A")


@pytest.fixture(scope="module")
def case_b():
    return Case("B")


def _wipe(table):
    return [np.nonzero(np.isin(CATS[table], WIPED[table]))[0]] * B0


def _per_category(c, m, exclude, nonempty):
    """{list: recommend(tup, m, exclude=, category=full(list), index=idx) on the host} for the lists with items"""
    return {l: [host(t) for t in c.m.recommend(c.tup, m, exclude=exclude, category=np.full(B0, l), index=c.idx)] for l in nonempty}


# ---- 1. the page against the per-category calls and the reference
@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (128, 4)])
@pytest.mark.parametrize("table", ["A", "B"])
def test_page_equals_the_per_category_calls_and_the_reference(table, d, H):
    c = Case(table, d, H)
    nonempty = [l for l, n in enumerate(TABLES[table]) if n]
    for exclude, sets in ((None, None), ("history", history_sets(c.b)), (_wipe(table), _wipe(table))):
        lids, lsc = ref.lists_of(c.sc_all, c.mask(exclude=sets), c.off, c.items, 64)
        calls = {}
        for S, m in PAGES:
            got = [host(t) for t in c.m.shelves(c.tup, S, m, index=c.idx, exclude=exclude)]
            cats, ids, sc = got
            assert cats.dtype == np.int32 and ids.dtype == np.int32 and sc.dtype == np.float32
            assert cats.shape == (B0, S) and ids.shape == (B0, S, m) and sc.shape == (B0, S, m)
            assert _equal(got, ref.page(lids, lsc, S, m)), (S, m, type(exclude))
            if m not in calls:
                calls[m] = _per_category(c, m, exclude, nonempty)
            for b in range(B0):
                for j in range(S):
                    if cats[b, j] < 0:
                        assert np.all(ids[b, j] == -1) and np.all(sc[b, j] == -np.inf)
                        continue
                    want = calls[m][int(cats[b, j])]
                    assert np.array_equal(ids[b, j], want[0][b]) and _same(sc[b, j], want[1][b]), (S, m, b, j)
            if exclude is None:
                full = min(S, len(nonempty))
                assert np.all(cats[:, :full] >= 0) and np.all(cats[:, full:] == -1), (S, m)
            elif not isinstance(exclude, str):
                assert not np.isin(cats, WIPED[table]).any()        # a list the exclusion empties is no shelf
            if table == "A" and S == 9:
                assert np.all(cats[:, 8] == -1)                     # only 8 lists hold items


# ---- 2. the plan decides the launch geometry, never the result
def test_plan_independence(case_b):
    c = case_b
    from tlsan_amd.model import shelves_plan
    lens = np.asarray(SIZES_B)
    so, sl, bo, bs = shelves_plan(lens, 300, 256)
    assert len(so) - 1 >= 3 and len(bo) - 1 == 2 and len(bs) == 3      # slices of 512: 600 -> 2, 257 -> 1
    so, sl, bo, bs = shelves_plan(lens, 64, 16)
    assert len(so) - 1 >= 3 and sorted(np.diff(bo).tolist())[-3:] == [1, 2, 3]    # slices of 256: 257 -> 2, 600 -> 3
    so, sl, bo, bs = shelves_plan(lens, 256, 0)
    assert len(sl) == 0 and len(bo) - 1 == 42                           # everything big
    for exclude in (None, "history"):
        for S, m, kw in ((5, 10, {}), (32, 8, {}), (4, 64, {}), (6, 20, dict(min_items=5, rank_at=4))):
            base = c.m.shelves(c.tup, S, m, index=c.idx, exclude=exclude, **kw)
            for plan in PLANS[1:]:
                assert _equal(c.m.shelves(c.tup, S, m, index=c.idx, exclude=exclude, **kw, **plan), base), (S, m, plan)


# ---- 3. ties and NaN
def test_ties_and_nan():
    in5, in7, in8 = (np.nonzero(CATS["A"] == l)[0] for l in (5, 7, 8))
    one = int(np.nonzero(CATS["A"] == 1)[0][0])
    x, y = int(in5[40]), int(in7[3])
    if x < y:                                        # the higher list holds the lower id
        x, y = int(in5[-1]), int(in7[0])
    assert y < x
    nan8, top8 = int(in8[20]), int(in8[5])

    def edit(p, b):
        p["item_emb"][y] = p["item_emb"][x]
        p["cate_emb"][7] = p["cate_emb"][5]
        p["item_b"][[x, y]] = 2000.0                 # the best item of lists 5 and 7: equal scores, bit for bit
        p["item_b"][one] = np.nan                    # the only item of list 1
        p["item_b"][nan8] = np.nan
        p["item_b"][top8] = 1000.0                   # list 8 is always the third shelf
        for k in ("i", "j", "hist_i", "hist_i_new"):
            b[k] = np.where(np.isin(b[k], [one, nan8]), 0, b[k])

    c = Case("A", edit=edit)
    cats, ids, sc = (host(t) for t in c.m.shelves(c.tup, 9, 3, index=c.idx))
    assert _equal((cats, ids, sc), ref.shelves(c.sc_all, c.mask(), c.off, c.items, 9, 3))
    assert np.all(cats[:, 0] == 7) and np.all(cats[:, 1] == 5) and np.all(cats[:, 2] == 8)       # equal scores: the lower item id
    assert np.all(ids[:, 0, 0] == y) and np.all(ids[:, 1, 0] == x) and np.array_equal(bits(sc[:, 0, 0]), bits(sc[:, 1, 0]))
    assert np.all(cats[:, 7] == 1) and np.all(ids[:, 7, 0] == one) and np.all(np.isnan(sc[:, 7, 0]))   # after every finite shelf
    assert np.all(np.isfinite(sc[:, :7, 0])) and np.all(cats[:, 8] == -1) and np.all(sc[:, 8] == -np.inf)   # before the padding
    cats, ids, sc = (host(t) for t in c.m.shelves(c.tup, 4, 39, index=c.idx))
    assert _equal((cats, ids, sc), ref.shelves(c.sc_all, c.mask(), c.off, c.items, 4, 39))
    assert np.all(cats[:, 2] == 8) and np.all(ids[:, 2, 38] == nan8) and np.all(np.isnan(sc[:, 2, 38]))   # NaN last in its shelf
    assert np.all(np.isfinite(sc[:, 2, :38]))


# ---- 4. min_items and rank_at
def test_min_items_and_rank_at():
    in3 = np.nonzero(CATS["A"] == 3)[0]

    def edit(p, b):
        b["hist_i"][0, 0] = in3[2]                   # row 0's history holds an item of the 16-item list (sl >= 1)

    c = Case("A", edit=edit)
    cats = host(c.m.shelves(c.tup, 9, 16, index=c.idx, min_items=16)[0])
    assert not np.isin(cats, [0, 1, 2]).any() and np.all((cats == 3).sum(1) == 1)
    assert np.all((cats >= 0).sum(1) == 6)
    sets = history_sets(c.b)
    got = c.m.shelves(c.tup, 9, 16, index=c.idx, min_items=16, exclude="history")
    assert _equal(got, ref.shelves(c.sc_all, c.mask(exclude=sets), c.off, c.items, 9, 16, min_items=16))
    cats = host(got[0])
    lost = np.array([bool(s & set(in3.tolist())) for s in sets])
    assert lost[0] and not lost.all() and np.array_equal((cats == 3).any(1), ~lost)
    pages = []
    for rank_at in (0, 9):
        got = c.m.shelves(c.tup, 5, 12, index=c.idx, min_items=10, rank_at=rank_at)
        assert _equal(got, ref.shelves(c.sc_all, c.mask(), c.off, c.items, 5, 12, min_items=10, rank_at=rank_at)), rank_at
        pages.append(host(got[0]))
        for plan in PLANS:                           # fewer shelves than a segment has candidates: full tables replace entries
            got = c.m.shelves(c.tup, 2, 12, index=c.idx, min_items=10, rank_at=rank_at, **plan)
            assert _equal(got, ref.shelves(c.sc_all, c.mask(), c.off, c.items, 2, 12, min_items=10, rank_at=rank_at)), (rank_at, plan)
    assert (pages[0] != pages[1]).any(1).sum() >= 1                  # the argument matters


# ---- 5. skip
def test_skip(case_b):
    c = case_b
    last = c.m.last_item_categories(c.tup)
    got = c.m.shelves(c.tup, 32, 8, index=c.idx, skip=last)
    lh = host(last)
    assert _equal(got, ref.shelves(c.sc_all, c.mask(), c.off, c.items, 32, 8, skip=lh))
    assert not (host(got[0]) == lh[:, None]).any()
    plain = host(c.m.shelves(c.tup, 32, 8, index=c.idx)[0])
    assert (plain == lh[:, None]).any()                               # without skip the row's own department is offered
    rng = np.random.RandomState(9)
    sk = plain[:, :3].copy().astype(np.int64)                         # each row's three best departments
    sk[rng.rand(B0, 3) < 0.3] = -1
    sk[::5, 1] = sk[::5, 0]                                           # repeats
    sk[3] = -7
    for S, m in ((4, 10), (32, 8)):
        got = c.m.shelves(c.tup, S, m, index=c.idx, skip=sk, exclude="history")
        assert _equal(got, ref.shelves(c.sc_all, c.mask(exclude=history_sets(c.b)), c.off, c.items, S, m, skip=sk)), (S, m)
        cats = host(got[0])
        assert not any(np.isin(cats[b], sk[b][sk[b] >= 0]).any() for b in range(B0))


# ---- 6. a row's page depends on its own inputs only
def test_independence_of_order_batch_and_repetition(case_b):
    c = case_b
    perm = np.random.RandomState(3).permutation(B0)
    last = host(c.m.last_item_categories(c.tup))
    for exclude in (None, "history"):
        for S, m in ((5, 10), (32, 8)):
            base = [host(t) for t in c.m.shelves(c.tup, S, m, index=c.idx, exclude=exclude, skip=last)]
            assert _equal(c.m.shelves(c.tup, S, m, index=c.idx, exclude=exclude, skip=last), base)
            shuffled = batch_tuple({k: v[perm] for k, v in c.b.items()}, True)
            assert _equal(c.m.shelves(shuffled, S, m, index=c.idx, exclude=exclude, skip=last[perm]), [t[perm] for t in base])
            for r in (0, 16, 17, 36):                                 # alone: B = 1
                one = batch_tuple({k: v[r:r + 1] for k, v in c.b.items()}, True)
                assert _equal(c.m.shelves(one, S, m, index=c.idx, exclude=exclude, skip=last[r:r + 1]), [t[r:r + 1] for t in base]), r


# ---- 7. the scope inside the index
def test_scope(case_a):
    c = case_a
    inside = np.arange(0, c.I, 3)
    sidx = c.m.category_index(within=c.m.item_scope(items=inside))
    off, items = lists_ref.index_of(c.cat, c.C, within=inside)
    for exclude, sets in ((None, None), ("history", history_sets(c.b))):
        for S, m in ((3, 10), (9, 10), (4, 64)):
            got = c.m.shelves(c.tup, S, m, index=sidx, exclude=exclude)
            assert _equal(got, ref.shelves(c.sc_all, c.mask(exclude=sets, within=inside), off, items, S, m)), (S, m)
            assert _equal(got, ref.shelves(c.sc_all, c.mask(exclude=sets, within=inside), c.off, c.items, S, m)), (S, m)
    empty = c.m.category_index(within=c.m.item_scope(items=[]))
    cats, ids, sc = (host(t) for t in c.m.shelves(c.tup, 3, 10, index=empty))
    assert np.all(cats == -1) and np.all(ids == -1) and np.all(sc == -np.inf)


# ---- 8. a hostile index through the raw helper
def test_hostile_index_entries_are_never_selected(case_a):
    import torch
    from tlsan_amd import model as M
    c = case_a
    I = c.I
    listed = np.array([-1, 0, 5, I + 5, 6, 300, I - 1, -1, 7, 8, I + 5, 9, 42, 42])   # lists of 4 / 5 / 3 entries, an empty one, and
    off = np.array([0, 4, 9, 12, 12, 13, 14])                                        # item 42 held by lists 4 and 5
    lists = (torch.as_tensor(off.astype(np.int32)).to(c.m.device), torch.as_tensor(np.concatenate([listed, [0]]).astype(np.int32)).to(c.m.device), 5)
    _, _, ut, db = c.m.forward(c.tup, is_test=True, want_u_t=True)
    for S, m in ((6, 3), (2, 1), (32, 8)):
        want = ref.shelves(c.sc_all, c.mask(), off, listed, S, m)
        for plan in (dict(), dict(seg_items=4, big_items=2), dict(seg_items=1, big_items=0), dict(seg_items=1, big_items=100)):
            got = M.shelves_topk(c.m.lib, c.m.dims, c.m.cparams, ut, db.B, S, m, 1, 0, (None, None), lists, None, 1, 0,
                                 c.m._topk_workspace, c.m._stream(), **plan)                 # (L.check: the call returned 0)
            assert _equal(got, want), (S, m, plan)
            cats, ids, _ = (host(t) for t in got)
            assert ids.max() < I and not (cats == 3).any()
            if S == 6:
                at = [int(np.nonzero(cats[b] == 4)[0][0]) for b in range(B0)]
                assert all(cats[b, at[b] + 1] == 5 and ids[b, at[b], 0] == 42 == ids[b, at[b] + 1, 0] for b in range(B0))


# ---- 9. lazy L2 and bf16 tables
@pytest.mark.parametrize("table_dtype", ["bf16", "f32"])
def test_lazy_l2_and_bf16_tables(table_dtype):
    cfg, m = lazy_model(1000, table_dtype, seed=41)            # d = 256, 31 categories, P != 1
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=43, test=True)
    tup = batch_tuple(b, True)
    idx = m.category_index()
    cat = host(m.item_cate)
    off, items = lists_ref.index_of(cat, 31)
    sc_all = host(m.score_candidates(tup, np.tile(np.arange(1000), (B0, 1))))
    for exclude, sets in ((None, None), ("history", history_sets(b))):
        ok = scope_ref.mask_of(B0, 1000, exclude=sets)
        for S, k in ((5, 10), (31, 8)):
            got = [host(t) for t in m.shelves(tup, S, k, index=idx, exclude=exclude)]
            assert _equal(got, ref.shelves(sc_all, ok, off, items, S, k)), (S, k, exclude)
            for l in np.unique(got[0][got[0] >= 0]):
                want = [host(t) for t in m.recommend(tup, k, exclude=exclude, category=np.full(B0, l), index=idx)]
                rows, js = np.nonzero(got[0] == l)
                assert np.array_equal(got[1][rows, js], want[0][rows]) and _same(got[2][rows, js], want[1][rows]), (S, k, l)


# ---- 10. state and composition
def test_state_is_read_not_changed_and_list_metrics_composes():
    import torch
    cfg = make_config(U=40, I=500, C=7, d=128, H=8)
    tb, cat = random_batch(cfg, B=64, Sn=3, seed=72)
    b, _ = random_batch(cfg, B=30, Sn=3, seed=73, test=True)
    m = model(cfg, cat, random_params(cfg, seed=71), l2_mode="lazy")
    for _ in range(3):
        m.train(None, batch_tuple(tb), 1.0)
    tup = batch_tuple(b, True)
    idx = m.category_index()
    m.shelves(tup, 3, 5, index=idx)                              # (what the last step owed lands with the first call)
    P = m.table_scale()
    assert P != 1.0
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.cate_emb, m.item_b, m.dense)]
    before = snap()
    m.shelves(tup, 4, 10, index=idx, exclude="history")
    m.shelves(tup, 7, 30, index=idx, min_items=3, rank_at=2, skip=m.last_item_categories(tup))
    cats, ids, _ = m.shelves(tup, 5, 8, index=idx, seg_items=64, big_items=16)
    assert m.table_scale() == P
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, snap()))
    res = m.list_metrics(ids.view(30, 40))
    assert int(res.n_cate.max()) <= 5 and int(res.n.max()) <= 40 and int(res.max_cate.max()) <= 8
    assert torch.equal(res.n_cate.long(), (cats >= 0).sum(1))    # a shelf holds one category, the shelves differ
    assert all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(before, snap()))


# ---- 11. the driver
def test_driver_writes_the_shelves(tmp_path):
    from tlsan_amd.model import Model
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    base = [sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "30", "--eval_freq", "1000",
            "--quiet", "--recommend_exclude", "none", "--shelves", "4", "--shelf_items", "5"]
    r = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--category_index" in r.stderr              # an argparse error
    r = subprocess.run(base + ["--category_index", "1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    page = np.load(os.path.join(out, "shelves_4x5.npz"))
    assert sorted(page.files) == ["cats", "ids", "scores", "users"]
    users, cats, ids, sc = (page[k] for k in ("users", "cats", "ids", "scores"))
    n = len(users)
    assert cats.shape == (n, 4) and ids.shape == (n, 4, 5) and sc.shape == (n, 4, 5) and cats.dtype == np.int32
    # the same run's model, reloaded: the file's shelves are its shelves, and each is recommend's list of that category
    from tlsan_amd import train as T
    train_set, test_set, (U, I, Cc), icl = T.load_dataset(ds)
    args = T.parse(["--dataset", ds, "--model_dir", out])
    config = {name: getattr(args, name) for name, _, _ in T.FLAGS}
    config.update(user_count=U, item_count=I, cate_count=Cc, from_scratch=False, quiet=True)
    m = Model(config, icl, device="cuda:0", seed=args.seed, norm_mode=args.norm_mode, l2_mode=args.l2_mode,
              table_dtype=args.table_dtype, matrix_dtype=args.matrix_dtype)
    m.restore(None, T.prepare_model_dir(out, False))
    idx = m.category_index()
    rows = T.EvalRows(test_set, config)
    at = 0
    for batch, real, _ in rows.launches(True):
        db = m.device_batch(batch, is_test=True)
        got = [host(t)[:real] for t in m.shelves(db, 4, 5, index=idx)]
        assert np.array_equal(users[at:at + real], host(db.u)[:real])
        assert _equal(got, (cats[at:at + real], ids[at:at + real], sc[at:at + real])), at
        for l in np.unique(got[0][got[0] >= 0]):
            want = [host(t)[:real] for t in m.recommend(db, 5, category=np.full(db.B, l), index=idx)]
            r_, j_ = np.nonzero(got[0] == l)
            assert np.array_equal(got[1][r_, j_], want[0][r_]) and _same(got[2][r_, j_], want[1][r_]), l
        at += real
    assert at == n

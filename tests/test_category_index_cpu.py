"""The per-category item index without a GPU: CategoryIndex and its per-shard local form against numpy, the ABI's three
additions (tlsan_lists_workspace_bytes / tlsan_eval_topk_lists / tlsan_similar_topk_lists) and every scalar refusal of
theirs (refused before any launch, on fake pointers that are never dereferenced), the argument checks of index= and
category= with it, the driver's flag, and the numpy reference of the contract (tests/lists_ref.py) on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import lists_ref, scope_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_lists_workspace_bytes", "tlsan_eval_topk_lists", "tlsan_similar_topk_lists")
CATE = np.array([2, 0, 2, 1, 0, 2, 4, 4, 0, 2, 5, 0, 2])      # 13 items in 7 categories; 3 and 6 are empty


def test_header_and_exports():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, hdr), name
        assert name in L.EXPORTS
        assert hasattr(L.load(), name)
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and L.load().tlsan_abi_version() == 15


def test_category_index_against_numpy():
    from tlsan_amd.model import CategoryIndex, ItemScope
    import torch
    for ic in (CATE, torch.as_tensor(CATE.astype(np.int32))):
        x = CategoryIndex(ic, 7, "cpu")
        off, items = lists_ref.index_of(CATE, 7)
        assert x.list_off.tolist() == off.tolist() and x.list_items.tolist() == items.tolist()
        assert str(x.list_off.dtype) == "torch.int32" and str(x.list_items.dtype) == "torch.int32"
        assert x.max_list == 5 and x.count == 13 and x.item_count == 13 and x.cate_count == 7
    assert off.tolist() == [0, 4, 5, 10, 10, 12, 13, 13]                # empty categories are empty lists
    assert items.tolist() == [1, 4, 8, 11, 3, 0, 2, 5, 9, 12, 6, 7, 10]  # ascending by (category, id)
    scope = ItemScope(13, "cpu", items=[12, 0, 3, 4, 6, 9])
    x = CategoryIndex(CATE, 7, "cpu", within=scope)
    off, items = lists_ref.index_of(CATE, 7, within=[0, 3, 4, 6, 9, 12])
    assert x.list_off.tolist() == off.tolist() == [0, 1, 2, 5, 5, 6, 6, 6]
    assert x.list_items.tolist() == items.tolist() == [4, 3, 0, 9, 12, 6]
    assert x.max_list == 3 and x.count == 6 and x.within is scope
    empty = CategoryIndex(CATE, 7, "cpu", within=ItemScope(13, "cpu", items=[]))
    assert empty.list_off.tolist() == [0] * 8 and empty.list_items.tolist() == [] and empty.max_list == 0
    for kw in (dict(item_cate=CATE, cate_count=4), dict(item_cate=CATE - 1, cate_count=7), dict(item_cate=CATE[None], cate_count=7),
               dict(item_cate=CATE.astype(np.float32), cate_count=7), dict(item_cate=CATE, cate_count=7, within=[1, 2]),
               dict(item_cate=CATE, cate_count=7, within=ItemScope(12, "cpu", items=[1]))):
        with pytest.raises(ValueError):
            CategoryIndex(device="cpu", **kw)


def test_category_index_local_form():
    from tlsan_amd.model import CategoryIndex, ItemScope
    for within in (None, [0, 3, 4, 6, 9, 12]):
        x = CategoryIndex(CATE, 7, "cpu", within=None if within is None else ItemScope(13, "cpu", items=within))
        goff, gitems = lists_ref.index_of(CATE, 7, within=within)
        off, items, longest = x.local(1, 0, 13)
        assert off.tolist() == goff.tolist() and items.tolist()[:-1] == gitems.tolist() and longest == np.diff(goff).max()
        assert items.numel() == len(gitems) + 1 and items.data_ptr() != 0       # one longer: an empty index has an address
        assert x.local(1, 0, 13)[0] is off                                      # cached per table
        for r in range(3):                              # rank r of 3 holds the ids g % 3 == r as local g // 3
            n = len(range(r, 13, 3))
            off, items, longest = x.local(3, r, n)
            held = [[g for g in gitems[goff[c]:goff[c + 1]] if g % 3 == r] for c in range(7)]
            assert np.diff(off.tolist()).tolist() == [len(h) for h in held]
            assert [i * 3 + r for i in items.tolist()[:-1]] == [g for h in held for g in h]
            assert longest == max(len(h) for h in held)
            for c in range(7):                          # ascending inside a list
                assert items.tolist()[off[c]:off[c + 1]] == sorted(items.tolist()[off[c]:off[c + 1]])
    off, items, longest = x.local(3, 1, 2)               # a table that ends before the scope does: ids 1, 4 only
    assert [i * 3 + 1 for i in items.tolist()[:-1]] == [4] and longest == 1


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

    need = lib.tlsan_lists_workspace_bytes(C.byref(dims), 4, 2, 16, 10, 50)
    assert need >= 200 * 4 and need < 200 * 128 * 4            # the inverse norms; no dense item matrix
    assert lib.tlsan_lists_workspace_bytes(C.byref(dims), 4, 2, 16, 10, 0) > 0      # an empty index is an index
    assert lib.tlsan_lists_workspace_bytes(C.byref(dims), 4, 8, 16, 10, 5000) > need
    for d, B, P, K, nl, ml in ((bad_dims, 4, 2, 16, 10, 50), (None, 4, 2, 16, 10, 50), (unsupported, 4, 2, 16, 10, 50),
                               (dims, 0, 2, 16, 10, 50), (dims, -1, 2, 16, 10, 50), (dims, 4, 0, 16, 10, 50),
                               (dims, 4, 9, 16, 10, 50), (dims, 4, 2, 0, 10, 50), (dims, 4, 2, 257, 10, 50),
                               (dims, 4, 2, 16, 0, 50), (dims, 4, 2, 16, 10, -1)):
        assert lib.tlsan_lists_workspace_bytes(ref_of(d), B, P, K, nl, ml) == 0, (B, P, K, nl, ml)
        assert b"tlsan_lists_workspace_bytes" in err(), err()

    def topk(d=dims, pp=p, ut=fake, B=4, K=16, off=None, xid=None, loff=fake, items=fake, nl=10, ml=50, rows=fake, P=2, mul=1,
             add=0, ids=fake, scores=fake, ws=fake, ws_bytes=1 << 40):
        return lib.tlsan_eval_topk_lists(ref_of(d), ref_of(pp), ut, B, K, off, xid, loff, items, nl, ml, rows, P, mul, add, ids,
                                         scores, ws, C.c_size_t(ws_bytes), None)

    def similar(d=dims, pp=p, qvec=fake, qinv=fake, qids=fake, Q=4, K=16, metric=L.SIM_COSINE, off=None, xid=None, loff=fake,
                items=fake, nl=10, ml=50, rows=fake, P=2, mul=1, add=0, ids=fake, scores=fake, ws=fake, ws_bytes=1 << 40):
        return lib.tlsan_similar_topk_lists(ref_of(d), ref_of(pp), qvec, qinv, qids, Q, K, metric, off, xid, loff, items, nl, ml,
                                            rows, P, mul, add, ids, scores, ws, C.c_size_t(ws_bytes), None)

    common = (dict(ids=None), dict(scores=None), dict(K=0), dict(K=257), dict(K=-1), dict(P=0), dict(P=9), dict(P=-1),
              dict(nl=0), dict(nl=-3), dict(ml=-1), dict(loff=None), dict(items=None), dict(rows=None), dict(d=None),
              dict(d=bad_dims), dict(pp=None), dict(pp=hole), dict(off=fake), dict(xid=fake), dict(mul=0), dict(add=-1),
              dict(mul=1 << 30))
    for kw in common + (dict(ut=None), dict(B=0), dict(B=-2)):
        assert topk(**kw) == -1, kw
        assert b"tlsan_eval_topk_lists" in err(), (kw, err())
    for kw in common + (dict(qvec=None), dict(qinv=None), dict(qids=None), dict(Q=0), dict(Q=-2), dict(metric=2), dict(metric=-1)):
        assert similar(**kw) == -1, kw
        assert b"tlsan_similar_topk_lists" in err(), (kw, err())
    for fn, name in ((topk, b"tlsan_eval_topk_lists"), (similar, b"tlsan_similar_topk_lists")):
        for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
            assert fn(**kw) == -2, kw
            assert name in err(), (kw, err())
        assert fn(d=unsupported) == -4 and name in err()
    assert similar(metric=L.SIM_DOT, qinv=None, ws_bytes=0) == -2      # (a NULL qinv is fine for dot: on to the workspace)


def test_python_argument_errors():
    from tlsan_amd.model import (CategoryIndex, ItemScope, index_categories, index_of, recommend_index, similar_index)
    idx = CategoryIndex(CATE, 7, "cpu")
    scope = ItemScope(13, "cpu", items=[1, 2])
    assert index_of(None, 13, 7) is None and index_of(idx, 13, 7) is idx
    for bad, I, Cn in ((idx, 12, 7), (idx, 13, 8), ([1, 2], 13, 7), (scope, 13, 7)):   # another item / category count, no index
        with pytest.raises(ValueError):
            index_of(bad, I, Cn)
    assert recommend_index(idx, None, 13, 7) is idx and recommend_index(None, scope, 13, 7) is None
    with pytest.raises(ValueError):
        recommend_index(idx, scope, 13, 7)                       # the scope belongs to the index
    with pytest.raises(ValueError):
        recommend_index(idx, None, 14, 7)
    assert similar_index(idx, None, True, 13, 7) is idx and similar_index(None, scope, False, 13, 7) is None
    for kw in (dict(within=None, same_category=False), dict(within=scope, same_category=True)):
        with pytest.raises(ValueError):
            similar_index(idx, item_count=13, cate_count=7, **kw)
    got = index_categories([4, -1, 0], 3, 7, "cpu")
    assert got.tolist() == [[4], [-1], [0]] and str(got.dtype) == "torch.int32" and got.is_contiguous()
    assert index_categories(np.array([[6, -9, 2], [0, 0, -1]]), 2, 7, "cpu").tolist() == [[6, -1, 2], [0, 0, -1]]
    assert index_categories(np.zeros((2, 8), np.int64), 2, 7, "cpu").shape == (2, 8)
    for bad, B in ((None, 3), ([7, 0, 0], 3), ([0, 0], 3), ([[0, 0, 0]], 3), ([0.0, 1.0, 2.0], 3), (np.zeros((3, 9), np.int64), 3),
                   (np.zeros((3, 0), np.int64), 3), (np.zeros((3, 2, 2), np.int64), 3), ([[0, 7], [0, 0], [1, 1]], 3),
                   ([True, False, True], 3)):
        with pytest.raises(ValueError):
            index_categories(bad, B, 7, "cpu")


def test_excl_rows():
    import torch
    from tlsan_amd.model import excl_rows
    assert excl_rows((None, None), torch.tensor([1]), 3) == (None, None)
    off = torch.arange(0, 16, 4, dtype=torch.int32)
    xid = torch.arange(12, dtype=torch.int32)
    o, x = excl_rows((off, xid), torch.tensor([2, 0]), 3)
    assert o.tolist() == [0, 4, 8] and x.tolist() == [8, 9, 10, 11, 0, 1, 2, 3] and str(o.dtype) == "torch.int32"


def test_reference_of_the_contract():
    off, items = lists_ref.index_of(CATE, 7)
    s = np.array([[0.5, 2.0, -0.0, 2.0, 7.0, 0.0, -1.0, 3.0, 0.5, 1.0, 9.0, 0.25, 1.0]], np.float32).repeat(5, 0)
    rows = [[2, 2, -1],        # a repeated probe counts once
            [-1, -1, -1],      # an all-negative row: nothing here (the caller runs it unrestricted)
            [3, 6, -1],        # empty lists only
            [4, 1, 0],         # a union of three lists
            [9, 5, 7]]         # ids past the index are no probe; 5 is the list [10]
    ok = lists_ref.union_mask(5, 13, rows, off, items, exclude=[set(), set(), set(), {4, 100, -2}, set()])
    assert ok.sum(1).tolist() == [5, 0, 0, 6, 1]
    ids, sc = scope_ref.topk(s, ok, 6)
    assert ids.tolist() == [[9, 12, 0, 2, 5, -1], [-1] * 6, [-1] * 6, [7, 1, 3, 8, 11, 6], [10, -1, -1, -1, -1, -1]]
    assert sc[0].tolist()[:5] == [1.0, 1.0, 0.5, 0.0, 0.0] and sc[0, 5] == -np.inf and not np.signbit(sc[0, 3])
    assert np.all(sc[1] == -np.inf) and sc[3].tolist() == [3.0, 2.0, 2.0, 0.5, 0.25, -1.0]
    # an entry of a list outside the table is not an item
    ok = lists_ref.union_mask(1, 13, [[0]], np.array([0, 4]), np.array([-1, 3, 13 + 5, 12]))
    assert np.nonzero(ok[0])[0].tolist() == [3, 12]
    # a [B] category array is the [B, 1] form, and equals scope_ref's category mask
    cat = np.array([2, -1, 3, 0, 5])
    assert np.array_equal(lists_ref.union_mask(5, 13, cat, off, items)[[0, 2, 3, 4]],
                          scope_ref.mask_of(5, 13, category=cat, item_cate=CATE)[[0, 2, 3, 4]])


def test_driver_checks_the_flag():
    from tlsan_amd import train as T
    assert T.parse(["--dataset", "x.npz"]).category_index == 0
    for good in (["--recommend_k", "5", "--recommend_same_category", "1"], ["--similar_k", "5", "--similar_same_category", "1"],
                 ["--recommend_k", "5", "--recommend_categories", "3,7", "--recommend_same_category", "1"],
                 ["--recommend_k", "5", "--recommend_categories", "3,7"]):
        assert T.parse(["--dataset", "x.npz", "--category_index", "1"] + good).category_index == 1
    for bad in (["--category_index", "1"], ["--category_index", "1", "--recommend_k", "5"],
                ["--category_index", "1", "--similar_k", "5"], ["--category_index", "2", "--recommend_k", "5",
                                                                "--recommend_same_category", "1"]):
        with pytest.raises(SystemExit):
            T.parse(["--dataset", "x.npz"] + bad)

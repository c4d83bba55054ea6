"""Scoped lists without a GPU: the ABI's additions, the argument checks of tlsan_scope_workspace_bytes /
tlsan_eval_topk_scoped / tlsan_similar_topk_scoped (refused before any launch, on fake pointers that are never
dereferenced), ItemScope and its per-shard local indices, last_item_categories, the reference's selection
(tests/scope_ref.py) on hand-made cases and the driver's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import scope_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_scope_workspace_bytes", "tlsan_eval_topk_scoped", "tlsan_similar_topk_scoped")


def test_header_and_exports():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, hdr), name
        assert name in L.EXPORTS
        assert hasattr(L.load(), name)
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and L.load().tlsan_abi_version() == 15


def test_arguments_are_refused_without_a_launch():
    from tlsan_amd import _lib as L
    lib = L.load()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    bad_dims = L.Dims(100, 200, 10, 128, 64, 32, 8, 10)       # d_item + d_cate != d
    unsupported = L.Dims(100, 200, 10, 96, 48, 48, 8, 10)     # a (d, heads) pair this build does not have
    fake = 0x1000                       # never dereferenced: every call below is refused by the argument checks
    p = L.Params(*([fake] * 8))
    hole = L.Params(*([fake] * 8))
    hole.item_cate = None
    err = lambda: lib.tlsan_last_error()
    ref_of = lambda d: C.byref(d) if d else None

    need = lib.tlsan_scope_workspace_bytes(C.byref(dims), 4, 16, 50)
    assert need >= 200 * 4                                     # the inverse norms; no dense item matrix
    assert need < 200 * 128 * 4
    assert lib.tlsan_scope_workspace_bytes(C.byref(dims), 4, 16, -1) >= need        # the whole table
    assert lib.tlsan_scope_workspace_bytes(C.byref(dims), 4, 16, 0) > 0             # an empty scope is a scope
    for d, B, K, nsub in ((bad_dims, 4, 16, 5), (None, 4, 16, 5), (unsupported, 4, 16, 5), (dims, 0, 16, 5), (dims, 4, 0, 5),
                          (dims, 4, 257, 5), (dims, 4, 16, 201)):
        assert lib.tlsan_scope_workspace_bytes(ref_of(d), B, K, nsub) == 0, (B, K, nsub)
        assert b"tlsan_scope_workspace_bytes" in err(), err()

    def topk(d=dims, pp=p, ut=fake, B=4, K=16, off=None, xid=None, sub=fake, nsub=50, cate=fake, mul=1, add=0, ids=fake,
             scores=fake, ws=fake, ws_bytes=1 << 40):
        return lib.tlsan_eval_topk_scoped(ref_of(d), ref_of(pp), ut, B, K, off, xid, sub, nsub, cate, mul, add, ids, scores,
                                          ws, C.c_size_t(ws_bytes), None)

    def similar(d=dims, pp=p, qvec=fake, qinv=fake, qids=fake, Q=4, K=16, metric=L.SIM_COSINE, off=None, xid=None, sub=fake,
                nsub=50, cate=fake, mul=1, add=0, ids=fake, scores=fake, ws=fake, ws_bytes=1 << 40):
        return lib.tlsan_similar_topk_scoped(ref_of(d), ref_of(pp), qvec, qinv, qids, Q, K, metric, off, xid, sub, nsub, cate,
                                             mul, add, ids, scores, ws, C.c_size_t(ws_bytes), None)

    scope = (dict(sub=None, nsub=0), dict(sub=None, nsub=7), dict(sub=fake, nsub=-1), dict(nsub=201), dict(sub=None, nsub=201))
    common = (dict(ids=None), dict(scores=None), dict(K=0), dict(K=257), dict(K=-1), dict(d=None), dict(d=bad_dims),
              dict(pp=None), dict(pp=hole), dict(off=fake), dict(xid=fake), dict(mul=0), dict(add=-1)) + scope
    for kw in common + (dict(ut=None), dict(B=0), dict(B=-2)):
        assert topk(**kw) == -1, kw
        assert b"tlsan_eval_topk_scoped" in err(), (kw, err())
    for kw in common + (dict(qvec=None), dict(qinv=None), dict(qids=None), dict(Q=0), dict(metric=2), dict(metric=-1)):
        assert similar(**kw) == -1, kw
        assert b"tlsan_similar_topk_scoped" in err(), (kw, err())
    for fn, name in ((topk, b"tlsan_eval_topk_scoped"), (similar, b"tlsan_similar_topk_scoped")):
        for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(sub=None, nsub=-1, ws_bytes=0)):
            assert fn(**kw) == -2, kw
            assert name in err(), (kw, err())
        assert fn(d=unsupported) == -4 and name in err()
    assert similar(metric=L.SIM_DOT, qinv=None, ws_bytes=0) == -2      # (a NULL qinv is fine for dot: on to the workspace)


def test_item_scope_construction():
    from tlsan_amd.model import ItemScope
    s = ItemScope(20, "cpu", items=[7, 3, 3, 19, 0])
    assert s.count == 4 and s.ids.tolist() == [0, 3, 7, 19] and str(s.ids.dtype) == "torch.int32"
    mask = np.zeros(20, bool)
    mask[[4, 5, 17]] = True
    assert ItemScope(20, "cpu", mask=mask).ids.tolist() == [4, 5, 17]
    cate = np.arange(20) % 4
    s = ItemScope(20, "cpu", categories=[1, 3], item_cate=cate)
    assert s.ids.tolist() == [n for n in range(20) if n % 4 in (1, 3)] and s.count == 10
    assert ItemScope(20, "cpu", items=[]).count == 0 and ItemScope(20, "cpu", mask=np.zeros(20, bool)).count == 0
    assert ItemScope(20, "cpu", categories=[9], item_cate=cate).count == 0
    for kw in (dict(items=[20]), dict(items=[-1, 2]), dict(items=[[1, 2]]), dict(items=[1.5]), dict(mask=np.zeros(19, bool)),
               dict(mask=np.zeros(20, np.int32)), dict(categories=[1]), dict(categories=[1], item_cate=cate[:5]), dict(),
               dict(items=[1], mask=mask)):
        with pytest.raises(ValueError):
            ItemScope(20, "cpu", **kw)


def test_item_scope_local_indices():
    from tlsan_amd.model import ItemScope
    ids = [0, 3, 4, 7, 8, 18, 19]
    s = ItemScope(20, "cpu", items=ids)
    whole = s.local(1, 0, 20)
    assert whole.tolist() == ids and s.sub(1, 0, 20)[0] is s.sub(1, 0, 20)[0]       # cached per table
    assert s.sub(1, 0, 20)[1] == 7 and s.sub(1, 0, 20)[0].data_ptr() != 0
    for r in (0, 1):                                    # rank r of 2 holds the ids g % 2 == r as local g // 2
        loc = s.local(2, r, 10)
        assert loc.tolist() == [g // 2 for g in ids if g % 2 == r]
        assert [n * 2 + r for n in loc.tolist()] == [g for g in ids if g % 2 == r]
    assert s.local(3, 1, 7).tolist() == [1, 2, 6]                                   # 4, 7, 19
    odd = ItemScope(20, "cpu", items=[1, 5])                                        # a scope that lies on one rank
    assert odd.local(2, 0, 10).tolist() == [] and odd.local(2, 1, 10).tolist() == [0, 2]
    assert odd.sub(2, 0, 10)[1] == 0 and odd.sub(2, 0, 10)[0].data_ptr() != 0       # an empty list still has an address
    empty = ItemScope(20, "cpu", items=[])
    assert empty.local(1, 0, 20).tolist() == [] and empty.sub(1, 0, 20)[0].data_ptr() != 0


def test_last_item_categories():
    import torch
    from tlsan_amd.model import DeviceBatch, last_item_categories
    hist_i = np.array([[5, 6, 0], [7, 0, 0], [0, 0, 0], [1, 2, 3]])
    hist_new = np.array([[9, 0], [0, 0], [4, 8], [0, 0]])
    sl, sl_new = np.array([2, 1, 0, 3]), np.array([1, 0, 2, 0])
    z = np.zeros(4, np.int64)
    db = DeviceBatch((z, z, z, hist_i, hist_new, np.zeros((4, 3), np.float32), sl, sl_new, z), "cpu", is_test=True)
    cate = torch.arange(10, dtype=torch.int32) + 100
    assert last_item_categories(db, cate).tolist() == [109, 107, 108, 103]
    db = DeviceBatch((z, z, z, hist_i, hist_new, np.zeros((4, 3), np.float32), sl * 0, sl_new * 0, z), "cpu", is_test=True)
    assert last_item_categories(db, cate).tolist() == [-1, -1, -1, -1]
    db = DeviceBatch((z, z, z, hist_i, np.zeros((4, 0), np.int64), np.zeros((4, 3), np.float32), sl, z, z), "cpu", is_test=True)
    assert last_item_categories(db, cate).tolist() == [106, 107, -1, 103]


def test_category_argument():
    from tlsan_amd.model import scope_categories
    assert scope_categories(None, 3, 5, "cpu") is None
    assert scope_categories([4, -1, 0], 3, 5, "cpu").tolist() == [4, -1, 0]
    assert scope_categories(np.array([-7, 2]), 2, 5, "cpu").tolist() == [-1, 2]
    for bad, B in (([5, 0, 0], 3), ([0, 0], 3), ([[0, 0, 0]], 3), ([0.0, 1.0, 2.0], 3)):
        with pytest.raises(ValueError):
            scope_categories(bad, B, 5, "cpu")


def test_reference_selection():
    nan = np.float32("nan")
    s = np.array([[0.5, 2.0, -0.0, 2.0, nan, 0.0, -1.0, nan, 0.5]], np.float32)
    ids, sc = ref.topk(s, np.ones((1, 9), bool), 10)
    assert ids.dtype == np.int32 and sc.dtype == np.float32
    assert ids[0].tolist() == [1, 3, 0, 8, 2, 5, 6, 4, 7, -1]            # ties by id; +0 == -0; NaN last, by id
    assert sc[0, 9] == -np.inf and np.isnan(sc[0, 7]) and np.isnan(sc[0, 8])
    assert sc[0, 4] == 0 and not np.signbit(sc[0, 4])                     # a zero score comes back as +0.0
    cate = np.array([0, 1, 1, 0, 1, 2, 2, 0, 1])
    ok = ref.mask_of(3, 9, within=[1, 3, 4, 5, 8], category=[1, -1, 7], item_cate=cate, exclude=[{8, 40, -3}, set(), set()])
    assert ok.tolist() == [[n in (1, 4) for n in range(9)], [n in (1, 3, 4, 5, 8) for n in range(9)], [False] * 9]
    ids, sc = ref.topk(np.repeat(s, 3, 0), ok, 3)
    assert ids.tolist() == [[1, 4, -1], [1, 3, 8], [-1, -1, -1]]
    assert sc[0, 0] == 2.0 and np.isnan(sc[0, 1]) and sc[0, 2] == -np.inf and np.all(sc[2] == -np.inf)
    assert sc[1].tolist() == [2.0, 2.0, 0.5]
    assert ref.mask_of(2, 4).all() and ref.mask_of(2, 4, within=[]).sum() == 0


def test_driver_checks_the_flags():
    from tlsan_amd import train as T
    args = T.parse(["--dataset", "x.npz"])
    assert args.recommend_categories == [] and args.recommend_same_category == 0 and args.similar_same_category == 0
    args = T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_categories", "3,7,12", "--recommend_same_category",
                    "1", "--similar_k", "4", "--similar_same_category", "1"])
    assert args.recommend_categories == [3, 7, 12] and args.recommend_same_category == 1 and args.similar_same_category == 1
    for bad in (["--recommend_categories", "3,7"], ["--recommend_same_category", "1"], ["--similar_same_category", "1"],
                ["--recommend_k", "5", "--similar_same_category", "1"], ["--similar_k", "5", "--recommend_same_category", "1"],
                ["--recommend_k", "5", "--recommend_categories", "3,x"], ["--recommend_k", "5", "--recommend_categories", "-2"],
                ["--recommend_k", "5", "--recommend_same_category", "2"]):
        with pytest.raises(SystemExit):
            T.parse(["--dataset", "x.npz"] + bad)
    assert T.recommend_path("m", 5) == os.path.join("m", "recommend_top5.npz")       # the lists keep their files
    assert T.similar_path("m", 4) == os.path.join("m", "similar-4.npz")

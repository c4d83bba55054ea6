"""The category shelves without a GPU: the numpy reference of the contract (tests/shelves_ref.py) on hand-made cases, the
ABI's two additions (tlsan_shelves_workspace_bytes / tlsan_eval_shelves) with every refusal of theirs (refused before any
launch, on fake pointers that are never dereferenced), the plan the host builds, the argument checks of Model.shelves (the
pure checking functions: the library is not touched), the sharded model's refusal and the driver's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import shelves_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_shelves_workspace_bytes", "tlsan_eval_shelves")


def test_header_exports_and_build_unit():
    from tlsan_amd import _lib as L, build
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, hdr), name
        assert name in L.EXPORTS
        assert hasattr(L.load(), name)
    assert "tlsan_shelves.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "tlsan_shelves.hip")) and os.path.exists(os.path.join(build.CSRC, "tlsan_shelves.h"))
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and L.load().tlsan_abi_version() == 15


# 10 items in 5 lists: list 3 is empty, lists 1 and 4 overlap in item 7
OFF = np.array([0, 3, 5, 9, 9, 10])
ITEMS = np.array([0, 1, 2, 7, 3, 4, 5, 6, 8, 7])
SCORES = np.array([[5.0, 4.0, 1.0, 0.5, 6.0, 3.0, 2.0, 9.0, -0.0, 0.0]], np.float32)


def test_reference_orders_shelves_by_rank_at():
    ok = np.ones((1, 10), bool)
    cats, ids, sc = ref.shelves(SCORES, ok, OFF, ITEMS, 5, 3)
    # best items: list 0 -> 5.0, list 1 -> 9.0 (item 7), list 2 -> 6.0, list 4 -> 9.0 (item 7): the tie goes to the lower list
    assert cats.tolist() == [[1, 4, 2, 0, -1]]
    assert ids[0].tolist() == [[7, 3, -1], [7, -1, -1], [4, 5, 6], [0, 1, 2], [-1, -1, -1]]
    assert sc[0, 0].tolist() == [9.0, 0.5, -np.inf] and sc[0, 4].tolist() == [-np.inf] * 3
    # ranked by the second entry: list 0 -> 4.0, list 1 -> 0.5, list 2 -> 3.0; list 4 has one item and is dropped
    cats, ids, _ = ref.shelves(SCORES, ok, OFF, ITEMS, 5, 3, min_items=2, rank_at=1)
    assert cats.tolist() == [[0, 2, 1, -1, -1]] and ids[0, 2].tolist() == [7, 3, -1]
    assert ref.shelves(SCORES, ok, OFF, ITEMS, 2, 3, min_items=3, rank_at=0)[0].tolist() == [[2, 0]]
    assert ref.shelves(SCORES, ok, OFF, ITEMS, 2, 3, min_items=3, rank_at=2)[0].tolist() == [[2, 0]]   # 2.0 before 1.0
    assert ref.shelves(SCORES, ok, OFF, ITEMS, 1, 1)[0].tolist() == [[1]]


def test_reference_min_items_counts_eligible_entries_and_skip():
    ok = np.ones((2, 10), bool)
    ok[1, [4, 7]] = False                              # row 1 has seen items 4 and 7
    s = SCORES.repeat(2, 0)
    cats, ids, _ = ref.shelves(s, ok, OFF, ITEMS, 5, 4, min_items=2)
    assert cats.tolist() == [[1, 2, 0, -1, -1], [0, 2, -1, -1, -1]]     # row 1: list 1 is left with one item, list 4 with none
    assert ids[1, 1].tolist() == [5, 6, 8, -1] and ids[0, 1].tolist() == [4, 5, 6, 8]
    cats, _, _ = ref.shelves(s, ok, OFF, ITEMS, 3, 2, skip=[1, 0])
    assert cats.tolist() == [[4, 2, 0], [2, 1, -1]]
    cats, _, _ = ref.shelves(s, ok, OFF, ITEMS, 3, 2, skip=[[1, 4, -1], [-1, -5, 2]])
    assert cats.tolist() == [[2, 0, -1], [0, 1, -1]]
    # an entry of a list outside the table is no item
    cats, ids, _ = ref.shelves(SCORES, np.ones((1, 10), bool), np.array([0, 3, 4]), np.array([-1, 12, 2, 9]), 2, 2)
    assert cats.tolist() == [[0, 1]] and ids[0].tolist() == [[2, -1], [9, -1]]


def test_reference_nan_last_and_zeros():
    s = np.array([[np.nan, 1.0, np.nan, -1e30, 2.0, 0.0, -0.0]], np.float32)
    off, items = np.array([0, 1, 3, 4, 7]), np.arange(7)
    cats, ids, sc = ref.shelves(s, np.ones((1, 7), bool), off, items, 5, 3)
    assert cats.tolist() == [[3, 1, 2, 0, -1]]         # the NaN shelf after every finite one, before the padding
    assert ids[0, 1].tolist() == [1, 2, -1] and np.isnan(sc[0, 1, 1])    # NaN last inside its shelf
    assert ids[0, 0].tolist() == [4, 5, 6] and not np.signbit(sc[0, 0, 2])   # +0 == -0: the lower id first, returned as +0.0
    assert np.isnan(sc[0, 3, 0]) and sc[0, 4, 0] == -np.inf


def test_plan_covers_every_list_once():
    from tlsan_amd.model import shelves_plan, shelves_thresholds, SHELF_SLICES_MAX
    lens = np.array([0, 1, 15, 255, 3, 0, 600, 257, 1, 40, 70000])
    for seg, big in ((300, 256), (64, 16), (256, 0), (1, 10 ** 9), (100000, 100000)):
        so, sl, bo, bs = shelves_plan(lens, seg, big)
        assert so.dtype == sl.dtype == bo.dtype == bs.dtype == np.int32 and bs.shape[1:] == (3,)
        assert so[0] == 0 and so[-1] == len(sl) and (np.diff(so) >= 1).all() and bo[0] == 0 and bo[-1] == len(bs)
        big_lists = [int(bs[bo[j], 0]) for j in range(len(bo) - 1)]
        assert sorted(sl.tolist() + big_lists) == np.flatnonzero(lens).tolist()
        assert all(lens[c] <= big for c in sl) and all(lens[c] > big for c in big_lists)
        assert sl.tolist() == sorted(sl.tolist())
        for s in range(len(so) - 1):                  # a segment stays within seg_items unless it is one list
            held = sl[so[s]:so[s + 1]]
            assert len(held) == 1 or lens[held].sum() <= seg
        for j in range(len(bo) - 1):                  # a big list's slices tile it
            cut = bs[bo[j]:bo[j + 1]]
            assert 1 <= len(cut) <= SHELF_SLICES_MAX and (cut[:, 0] == cut[0, 0]).all() and cut[0, 1] == 0
            assert (cut[1:, 1] == cut[:-1, 2]).all() and cut[-1, 2] == lens[cut[0, 0]] and (cut[:, 2] > cut[:, 1]).all()
    so, sl, bo, bs = shelves_plan(np.zeros(4, np.int64), 300, 256)
    assert so.tolist() == [0] and bo.tolist() == [0] and len(sl) == 0 and bs.shape == (0, 3)
    for bad in ((0, 5), (10, -1)):
        with pytest.raises(ValueError):
            shelves_plan(lens, *bad)
    for total, B in ((1200, 37), (63001, 4096), (5 * 10 ** 6, 4096), (5 * 10 ** 6, 1), (0, 1)):
        seg, big = shelves_thresholds(total, B)
        assert seg >= 1024 and seg % 256 == 0 and big == 4 * seg and -(-total // seg) <= 1024


def test_workspace_grows_with_every_argument():
    from tlsan_amd import _lib as L
    lib = L.load()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    size = lambda B=37, S=4, m=10, nseg=3, nbig=2, nbs=5: lib.tlsan_shelves_workspace_bytes(C.byref(dims), B, S, m, nseg, nbig, nbs)
    base = size()
    assert base >= 37 * (3 * 4 + 5) * 10 * 8
    assert size(nseg=0, nbig=0, nbs=0) > 0                               # an empty index is an index
    assert size(B=1 << 24, S=32, m=8, nseg=32767, nbig=32767, nbs=32767) > base
    for kw in (dict(B=38), dict(S=5), dict(m=11), dict(nseg=4), dict(nbig=3, nbs=6), dict(nbs=6)):
        assert size(**kw) > base, kw
    for kw in (dict(B=36), dict(S=3), dict(m=9), dict(nseg=2), dict(nbig=1, nbs=4)):
        assert size(**kw) <= base, kw


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

    for d, B, S, m, nseg, nbig, nbs in ((bad_dims, 4, 4, 10, 3, 2, 5), (None, 4, 4, 10, 3, 2, 5), (unsupported, 4, 4, 10, 3, 2, 5),
                                        (dims, 0, 4, 10, 3, 2, 5), (dims, -1, 4, 10, 3, 2, 5), (dims, (1 << 24) + 1, 4, 10, 3, 2, 5),
                                        (dims, 4, 0, 10, 3, 2, 5), (dims, 4, 33, 8, 3, 2, 5), (dims, 4, 4, 0, 3, 2, 5),
                                        (dims, 4, 4, 65, 3, 2, 5), (dims, 4, 5, 52, 3, 2, 5), (dims, 4, 32, 9, 3, 2, 5),
                                        (dims, 4, 4, 10, -1, 2, 5), (dims, 4, 4, 10, 32768, 2, 5), (dims, 4, 4, 10, 3, -1, 5),
                                        (dims, 4, 4, 10, 3, 2, 1), (dims, 4, 4, 10, 3, 2, 33), (dims, 4, 4, 10, 3, 0, 1),
                                        (dims, 4, 4, 10, 3, 32768, 32768)):
        assert lib.tlsan_shelves_workspace_bytes(ref_of(d), B, S, m, nseg, nbig, nbs) == 0, (B, S, m, nseg, nbig, nbs)
        assert b"tlsan_shelves_workspace_bytes" in err(), err()
    need = lib.tlsan_shelves_workspace_bytes(C.byref(dims), 4, 4, 10, 3, 2, 5)
    assert need > 0

    def call(d=dims, pp=p, ut=fake, B=4, S=4, m=10, mi=2, ra=1, off=None, xid=None, loff=fake, items=fake, nl=10, ml=50, so=fake,
             sl=fake, nseg=3, nsmall=8, bo=fake, bs=fake, nbig=2, nbs=5, skip=None, X=0, mul=1, add=0, cats=fake, ids=fake, scores=fake,
             ws=fake, ws_bytes=1 << 40):
        return lib.tlsan_eval_shelves(ref_of(d), ref_of(pp), ut, B, S, m, mi, ra, off, xid, loff, items, nl, ml, so, sl, nseg, nsmall,
                                      bo, bs, nbig, nbs, skip, X, mul, add, cats, ids, scores, ws, C.c_size_t(ws_bytes), None)

    badarg = (dict(d=None), dict(d=bad_dims), dict(pp=None), dict(pp=hole), dict(ut=None), dict(cats=None), dict(ids=None),
              dict(scores=None), dict(B=0), dict(B=-2), dict(B=(1 << 24) + 1), dict(S=0), dict(S=33, m=7), dict(S=-1), dict(m=0),
              dict(m=65), dict(S=5, m=52), dict(S=32, m=9), dict(mi=0), dict(mi=11), dict(mi=-1), dict(ra=-1), dict(ra=2),
              dict(mi=1, ra=1), dict(nl=0), dict(nl=-3), dict(nl=(1 << 24) + 1), dict(ml=-1), dict(loff=None), dict(items=None),
              dict(so=None), dict(sl=None), dict(bo=None), dict(bs=None), dict(nseg=-1), dict(nseg=32768), dict(nsmall=-1),
              dict(nsmall=0), dict(nbig=-1), dict(nbs=1), dict(nbs=33), dict(nbig=0, nbs=1), dict(skip=fake), dict(X=1),
              dict(skip=fake, X=9), dict(skip=fake, X=-1), dict(off=fake), dict(xid=fake), dict(mul=0), dict(add=-1),
              dict(mul=1 << 30))
    for kw in badarg:
        assert call(**kw) == -1, kw
        assert b"tlsan_eval_shelves" in err(), (kw, err())
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**kw) == -2, kw
        assert b"tlsan_eval_shelves" in err(), (kw, err())
    assert call(d=unsupported) == -4 and b"tlsan_eval_shelves" in err()
    # what is allowed reaches the workspace check: a plan without segments or without big lists, skip with X
    for kw in (dict(so=None, sl=None, nseg=0, nsmall=0), dict(bo=None, bs=None, nbig=0, nbs=0), dict(skip=fake, X=8),
               dict(off=fake, xid=fake), dict(S=32, m=8, mi=8, ra=7), dict(S=4, m=64, mi=1, ra=0)):
        assert call(ws_bytes=0, **kw) == -2, kw


def test_python_argument_errors():
    import torch
    from tlsan_amd.model import CategoryIndex, ItemScope, Model, shelves_index, shelves_sizes, shelves_skip
    assert shelves_sizes(4, 10, 1, 0) == (4, 10, 1, 0) and shelves_sizes(np.int64(32), 8, 8, 7) == (32, 8, 8, 7)
    assert shelves_sizes(4, 64, 64, 63) == (4, 64, 64, 63) and shelves_sizes(1, 1, 1, 0) == (1, 1, 1, 0)
    for bad in ((0, 10, 1, 0), (33, 7, 1, 0), (4, 0, 1, 0), (4, 65, 1, 0), (5, 52, 1, 0), (32, 9, 1, 0), (4, 10, 0, 0),
                (4, 10, 11, 0), (4, 10, 2, 2), (4, 10, 1, 1), (4, 10, 1, -1), (2.5, 10, 1, 0), (4, True, 1, 0), (-1, 10, 1, 0)):
        with pytest.raises(ValueError):
            shelves_sizes(*bad)
    cate = np.array([2, 0, 2, 1, 0, 2, 4, 4, 0, 2, 5, 0, 2])
    idx = CategoryIndex(cate, 7, "cpu")
    assert shelves_index(idx, 13, 7) is idx
    for bad, I, Cn in ((None, 13, 7), (idx, 12, 7), (idx, 13, 8), ([1, 2], 13, 7), (ItemScope(13, "cpu", items=[1]), 13, 7)):
        with pytest.raises(ValueError):
            shelves_index(bad, I, Cn)
    assert shelves_skip(None, 3, 7, "cpu") is None
    got = shelves_skip([4, -9, 0], 3, 7, "cpu")
    assert got.tolist() == [[4], [-1], [0]] and str(got.dtype) == "torch.int32" and got.is_contiguous()
    assert shelves_skip(torch.tensor([[6, -1, 2], [0, 0, -1]]), 2, 7, "cpu").tolist() == [[6, -1, 2], [0, 0, -1]]
    assert shelves_skip(np.zeros((2, 8), np.int64), 2, 7, "cpu").shape == (2, 8)
    for bad, B in (([7, 0, 0], 3), ([0, 0], 3), ([[0, 0, 0]], 3), ([0.0, 1.0, 2.0], 3), (np.zeros((3, 9), np.int64), 3),
                   (np.zeros((3, 0), np.int64), 3), (np.zeros((3, 2, 2), np.int64), 3), ([[0, 7], [0, 0], [1, 1]], 3),
                   ([True, False, True], 3)):
        with pytest.raises(ValueError):
            shelves_skip(bad, B, 7, "cpu")

    class Stub:                                         # Model.shelves checks everything before it touches the library
        config = dict(item_count=13, cate_count=7)
        device = "cpu"

        def forward(self, *a, **k):
            raise AssertionError("a refused call went on to the forward pass")

    batch = (np.zeros(3),)
    for kw in (dict(shelves=0, k=5, index=idx), dict(shelves=33, k=5, index=idx), dict(shelves=4, k=65, index=idx),
               dict(shelves=16, k=17, index=idx), dict(shelves=4, k=5), dict(shelves=4, k=5, index=CategoryIndex(cate[:12], 7, "cpu")),
               dict(shelves=4, k=5, index=CategoryIndex(cate, 8, "cpu")), dict(shelves=4, k=5, index=idx, min_items=6),
               dict(shelves=4, k=5, index=idx, min_items=2, rank_at=2), dict(shelves=4, k=5, index=idx, rank_at=1),
               dict(shelves=4, k=5, index=idx, skip=[0, 1]), dict(shelves=4, k=5, index=idx, skip=[0, 7, 1]),
               dict(shelves=4, k=5, index=idx, skip=np.zeros((3, 9), np.int64))):
        with pytest.raises(ValueError):
            Model.shelves(Stub(), batch, **kw)
    for name in ("boost", "diversity", "within", "category"):
        with pytest.raises(TypeError):
            Model.shelves(Stub(), batch, 4, 5, index=idx, **{name: None})
        assert name in Model.shelves.__doc__              # the docstring says what is out of scope


def test_sharded_model_refuses():
    from tlsan_amd.dist import ShardedModel
    with pytest.raises(NotImplementedError, match="spread over the ranks"):
        ShardedModel.shelves(object(), None, 4, 5)


def test_driver_checks_the_flags(monkeypatch):
    from tlsan_amd import train as T
    a = T.parse(["--dataset", "x.npz", "--category_index", "1", "--shelves", "4", "--shelf_items", "5"])
    assert (a.shelves, a.shelf_items, a.shelf_min_items, a.shelf_skip_last) == (4, 5, 1, 0)
    a = T.parse(["--dataset", "x.npz", "--category_index", "1", "--shelves", "32", "--shelf_items", "8", "--shelf_min_items", "8",
                 "--shelf_skip_last", "1", "--recommend_exclude", "none"])
    assert (a.shelves, a.shelf_items, a.shelf_min_items, a.shelf_skip_last) == (32, 8, 8, 1)
    assert T.parse(["--dataset", "x.npz"]).shelves == 0
    assert T.shelves_path("d", 4, 5) == os.path.join("d", "shelves_4x5.npz")
    for bad in (["--shelves", "4", "--shelf_items", "5"], ["--category_index", "1", "--shelves", "4"],
                ["--category_index", "1", "--shelf_items", "5", "--recommend_k", "5", "--recommend_same_category", "1"],
                ["--category_index", "1", "--shelves", "33", "--shelf_items", "5"], ["--category_index", "1", "--shelves", "4", "--shelf_items", "65"],
                ["--category_index", "1", "--shelves", "32", "--shelf_items", "9"],
                ["--category_index", "1", "--shelves", "4", "--shelf_items", "5", "--shelf_min_items", "6"],
                ["--category_index", "1", "--shelves", "4", "--shelf_items", "5", "--shelf_skip_last", "2"],
                ["--category_index", "1", "--shelves", "4", "--shelf_items", "5", "--sharded", "1"],
                ["--category_index", "1", "--shelf_skip_last", "1", "--recommend_k", "5", "--recommend_same_category", "1"]):
        with pytest.raises(SystemExit):
            T.parse(["--dataset", "x.npz"] + bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        T.parse(["--dataset", "x.npz", "--category_index", "1", "--shelves", "4", "--shelf_items", "5"])

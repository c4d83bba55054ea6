"""Boosted lists without a GPU: the reference (tests/boost_ref.py) against a brute-force Python sort on tiny inputs with
NaN, signed zeros, -inf, exact ties and k past the eligible count; the ABI's two additions (tlsan_eval_topk_scoped_boost,
tlsan_eval_topk_lists_boost) and their refusals -- every refusal of the unboosted call with the same code and the boosted
function's name, and a NULL boost, all before any launch on fake pointers that are never dereferenced; ItemBoost's
constructors and sum on "cpu"; recommend's argument checks; and the driver's two flags with the vector they build."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from tests import boost_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_eval_topk_scoped_boost", "tlsan_eval_topk_lists_boost")


# ---- the reference
def _brute(adj_row, ids, k, excluded_row):
    """one row by Python's sort with the order written out as a comparison"""
    def cmp(a, b):
        (sa, ga), (sb, gb) = a, b
        na, nb = math.isnan(sa), math.isnan(sb)
        if na != nb:
            return 1 if na else -1              # NaN after everything else
        if not na and sa != sb:                 # (+0.0 == -0.0 in Python as in IEEE)
            return -1 if sa > sb else 1         # higher first
        return -1 if ga < gb else (1 if ga > gb else 0)
    cand = [(float(s), int(g)) for s, g, x in zip(adj_row, ids, excluded_row) if not x]
    cand.sort(key=functools.cmp_to_key(cmp))
    return cand[:k]


def test_adjusted_is_two_float32_roundings():
    s = np.array([[1.0, 1.0, -0.0, 3.0]], np.float32)
    b = np.array([2.0 ** -24, 2.0 ** -23, 0.0, -np.inf], np.float32)
    out = ref.adjusted(s, b)
    assert out.dtype == np.float32 and out[0, 0] == 1.0 and out[0, 1] == np.float32(1.0 + 2.0 ** -23) and out[0, 3] == -np.inf
    # with a weight the product is rounded before the sum: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11, and
    # -1 - 2^-11 + that is 0 -- a fused multiply-add would leave 2^-24
    w = np.array([1.0 + 2.0 ** -12], np.float32)
    b2 = np.array([1.0 + 2.0 ** -12], np.float32)
    s2 = np.array([[-(1.0 + 2.0 ** -11)]], np.float32)
    assert ref.adjusted(s2, b2, w)[0, 0] == 0.0
    assert float(np.float64(w[0]) * np.float64(b2[0]) + np.float64(s2[0, 0])) == 2.0 ** -24
    with np.errstate(all="ignore"):
        assert np.isnan(ref.adjusted(s, b, np.array([0.0], np.float32))[0, 3])          # 0 * inf = NaN
    assert np.array_equal(ref.adjusted(s, np.zeros(4, np.float32), np.array([7.0], np.float32)).view(np.int32)[0, [0, 1, 3]],
                          s.view(np.int32)[0, [0, 1, 3]])


def test_reference_selection_against_a_python_sort():
    nan, inf = np.float32("nan"), np.float32("inf")
    rng = np.random.RandomState(5)
    pool = np.array([nan, 0.0, -0.0, -inf, inf, 1.5, 1.5, -2.0, 0.25, 0.25, 0.25, 3.0], np.float32)
    for trial in range(40):
        n = int(rng.randint(1, 14))
        ids = np.sort(rng.choice(50, n, replace=False))
        adj = pool[rng.randint(0, len(pool), (3, n))]
        excluded = rng.rand(3, n) < 0.25 if trial % 2 else None
        for k in (1, 4, 20):                                                   # (20: past every eligible count)
            got_ids, got_sc = ref.topk(adj, ids, k, excluded)
            assert got_ids.dtype == np.int32 and got_sc.dtype == np.float32 and got_ids.shape == (3, k)
            for r in range(3):
                want = _brute(adj[r], ids, k, np.zeros(n, bool) if excluded is None else excluded[r])
                assert got_ids[r, :len(want)].tolist() == [g for _, g in want], (trial, k, r)
                assert np.all(got_ids[r, len(want):] == -1) and np.all(got_sc[r, len(want):] == -np.inf)
                for j, (s, _) in enumerate(want):
                    assert (math.isnan(s) and np.isnan(got_sc[r, j])) or got_sc[r, j] == s, (trial, k, r, j)
                    assert not (got_sc[r, j] == 0 and np.signbit(got_sc[r, j]))     # a zero comes back as +0.0
    ids, sc = ref.topk(np.array([[nan, -inf, -0.0, 0.0, 2.0, 2.0]], np.float32), np.array([9, 8, 7, 3, 5, 4]), 8)
    assert ids[0].tolist() == [4, 5, 3, 7, 8, 9, -1, -1]                        # ties by id; -inf before NaN; then the padding
    assert np.isnan(sc[0, 5]) and sc[0, 4] == -np.inf and sc[0, 6] == -np.inf


# ---- the ABI
def test_header_and_exports():
    from tlsan_amd import _lib as L, build
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    lib = L.load()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert re.search(r"const float\*\s+boost,\s*const float\*\s+row_weight\s*$", m.group(1)), name
        assert name in L.EXPORTS and hasattr(lib, name)
    assert "tlsan_boost.hip" in build.SOURCES
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

    def scoped(boosted, d=dims, pp=p, ut=fake, B=4, K=16, off=None, xid=None, sub=fake, nsub=50, cate=fake, mul=1, add=0, ids=fake,
               scores=fake, ws=fake, ws_bytes=1 << 40, boost=fake, weight=None):
        args = (ref_of(d), ref_of(pp), ut, B, K, off, xid, sub, nsub, cate, mul, add, ids, scores, ws, C.c_size_t(ws_bytes), None)
        return lib.tlsan_eval_topk_scoped_boost(*args, boost, weight) if boosted else lib.tlsan_eval_topk_scoped(*args)

    def lists(boosted, d=dims, pp=p, ut=fake, B=4, K=16, off=None, xid=None, loff=fake, items=fake, nl=10, ml=50, rows=fake, P=2,
              mul=1, add=0, ids=fake, scores=fake, ws=fake, ws_bytes=1 << 40, boost=fake, weight=None):
        args = (ref_of(d), ref_of(pp), ut, B, K, off, xid, loff, items, nl, ml, rows, P, mul, add, ids, scores, ws,
                C.c_size_t(ws_bytes), None)
        return lib.tlsan_eval_topk_lists_boost(*args, boost, weight) if boosted else lib.tlsan_eval_topk_lists(*args)

    need_s = lib.tlsan_scope_workspace_bytes(C.byref(dims), 4, 16, 50)
    need_l = lib.tlsan_lists_workspace_bytes(C.byref(dims), 4, 2, 16, 10, 50)
    shared = (dict(ids=None), dict(scores=None), dict(ut=None), dict(B=0), dict(B=-2), dict(K=0), dict(K=257), dict(K=-1),
              dict(d=None), dict(d=bad_dims), dict(d=unsupported), dict(pp=None), dict(pp=hole), dict(off=fake), dict(xid=fake),
              dict(mul=0), dict(add=-1), dict(mul=1 << 30), dict(ws=None), dict(ws_bytes=0))
    scoped_only = (dict(sub=None, nsub=0), dict(sub=None, nsub=7), dict(sub=fake, nsub=-1), dict(nsub=201), dict(sub=None, nsub=201),
                   dict(ws_bytes=need_s - 1), dict(sub=None, nsub=-1, ws_bytes=0))
    lists_only = (dict(P=0), dict(P=9), dict(P=-1), dict(nl=0), dict(nl=-3), dict(nl=(1 << 24) + 1), dict(B=(1 << 24) + 1),
                  dict(ml=-1), dict(loff=None), dict(items=None), dict(rows=None), dict(ws_bytes=need_l - 1))
    for fn, name, cases in ((scoped, NAMES[0], shared + scoped_only), (lists, NAMES[1], shared + lists_only)):
        for kw in cases:
            for weight in (None, fake):
                plain = fn(False, **kw)
                assert plain in (-1, -2, -4), (name, kw, plain)                  # BADARG, WORKSPACE, UNSUPPORTED: refused
                assert fn(True, weight=weight, **kw) == plain, (name, kw)        # the same code ...
                assert name.encode() in err(), (name, kw, err())                 # ... under the boosted function's name
        assert fn(True, boost=None) == -1 and name.encode() in err() and b"boost" in err()
        assert fn(True, boost=None, weight=fake) == -1 and name.encode() in err()
        assert fn(True, boost=None, ws_bytes=0) == -1                            # (a NULL boost is refused ahead of the workspace)


# ---- ItemBoost
def test_item_boost_construction_and_sum():
    import torch
    from tlsan_amd.model import ItemBoost, item_boost_for
    b = ItemBoost([0.5, -1, 2, 0], device="cpu")
    assert b.item_count == 4 and b.values.dtype == torch.float32 and b.values.tolist() == [0.5, -1.0, 2.0, 0.0]
    assert ItemBoost(np.arange(3)).values.tolist() == [0.0, 1.0, 2.0]            # integers are numbers
    t = torch.tensor([1.0, float("-inf"), float("nan")], dtype=torch.float64)
    v = ItemBoost(t).values
    assert v.dtype == torch.float32 and v[0] == 1 and v[1] == float("-inf") and torch.isnan(v[2])
    for bad in ([[1.0, 2.0]], [], np.zeros(3, bool), 1.0):
        with pytest.raises(ValueError):
            ItemBoost(bad)
    o = ItemBoost.of_items(6, [4, 1, 4], [1.0, 2.0, 3.0], base=-0.5)
    assert o.values.tolist() == [-0.5, 2.0, -0.5, -0.5, 3.0, -0.5]                # an id named twice keeps its last value
    assert ItemBoost.of_items(4, np.array([0, 3]), 2 ** 20).values.tolist() == [2.0 ** 20, 0.0, 0.0, 2.0 ** 20]
    assert ItemBoost.of_items(3, [], []).values.tolist() == [0.0, 0.0, 0.0]
    for ids, vals in (([6], [1.0]), ([-1], [1.0]), ([1, 2], [1.0]), ([[1]], [1.0]), ([1.5], [1.0])):
        with pytest.raises(ValueError):
            ItemBoost.of_items(6, ids, vals)
    cate = np.array([2, 0, 1, 2, 2, 0])
    c = ItemBoost.of_categories([10.0, 20.0, float("-inf")], cate)
    assert c.values.tolist() == [float("-inf"), 10.0, 20.0, float("-inf"), float("-inf"), 10.0]
    assert ItemBoost.of_categories(torch.tensor([1.0, 2.0, 3.0]), torch.as_tensor(cate)).values.tolist() == [3.0, 1.0, 2.0, 3.0, 3.0, 1.0]
    for cv, ic in (([1.0, 2.0], cate), ([1.0, 2.0, 3.0], -cate), ([1.0, 2.0, 3.0], cate.astype(np.float32)), ([[1.0]], cate)):
        with pytest.raises(ValueError):
            ItemBoost.of_categories(cv, ic)
    big, small = ItemBoost([1.0, 16777216.0]), ItemBoost([2.0 ** -24, 1.0])
    s = big + small
    assert isinstance(s, ItemBoost) and s.values.tolist() == [1.0, 16777216.0]   # an fp32 sum: both addends are lost
    assert (o + ItemBoost.of_categories([1.0, 2.0, 3.0], cate)).values.tolist() == [2.5, 3.0, 1.5, 2.5, 6.0, 0.5]
    with pytest.raises(ValueError):
        o + b
    with pytest.raises(TypeError):
        o + 1.0
    # the models' convenience: exactly one of values / items / categories, the count and the device filled in
    icl = lambda: torch.as_tensor(cate)
    assert item_boost_for(6, "cpu", icl, [0, 1, 2, 3, 4, 5], None, None, 0.0).item_count == 6
    assert item_boost_for(6, "cpu", icl, None, ([2], [7.0]), None, 1.0).values.tolist() == [1.0, 1.0, 7.0, 1.0, 1.0, 1.0]
    assert item_boost_for(6, "cpu", icl, None, None, [1.0, 2.0, 3.0], 0.0).values.tolist() == [3.0, 1.0, 2.0, 3.0, 3.0, 1.0]
    for args in (([0, 1, 2], None, None), (None, None, None), ([0] * 6, ([1], [1.0]), None)):
        with pytest.raises(ValueError):
            item_boost_for(6, "cpu", icl, *args, 0.0)


def test_recommend_argument_checks():
    import torch
    from tlsan_amd.model import ItemBoost, boost_of
    assert boost_of(None, None, 5, 9, "cpu") is None
    v, w = boost_of(np.arange(9), None, 5, 9, "cpu")
    assert v.dtype == torch.float32 and v.tolist() == list(range(9)) and w is None
    held = ItemBoost(np.arange(9))
    v, w = boost_of(held, [0, 1, -1, 0.5, 2], 5, 9, "cpu")
    assert v.data_ptr() == held.values.data_ptr()                                # a holder is reused, not copied
    assert w.dtype == torch.float32 and w.tolist() == [0.0, 1.0, -1.0, 0.5, 2.0]
    for boost, weight in ((None, [1.0] * 5), (np.arange(8), None), (held, [1.0] * 4), (held, [[1.0] * 5]), (held, 1.0),
                          (ItemBoost(np.arange(10)), None)):
        with pytest.raises(ValueError):
            boost_of(boost, weight, 5, 9, "cpu")


# ---- the driver
def test_driver_flags_and_vector(tmp_path):
    from tlsan_amd import train as T
    from tlsan_amd.input import PackedSet, item_self_information
    args = T.parse(["--dataset", "x.npz"])
    assert args.recommend_boost == "" and args.recommend_novelty == 0.0
    assert T.recommend_boost_vector(args, None, 6) is None
    for bad in (["--recommend_boost", "b.npy"], ["--recommend_novelty", "0.5"], ["--recommend_k", "5", "--recommend_novelty", "x"],
                ["--recommend_k", "5", "--shortlist_index", "1", "--recommend_novelty", "0.5"]):
        with pytest.raises(SystemExit):
            T.parse(["--dataset", "x.npz"] + bad)
    I = 6
    # five samples: positives 1, 1, 4 (label 1); targets 2, 1 are sampled negatives (label 0)
    train = PackedSet.from_samples([(0, [1], [2], [0.0], 1, 1, 0), (1, [], [1], [], 1, 1, 0), (0, [1, 2], [0], [0.0, 1.0], 4, 1, 0),
                                    (2, [3], [3], [0.0], 2, 0, 1), (1, [0], [2], [0.0], 1, 0, 1)])
    info = item_self_information(train, I)
    path = str(tmp_path / "boost.npy")
    file_vals = np.array([0.0, -np.inf, 2.0 ** 20, 1.0, -1.0, 0.5], np.float32)
    np.save(path, file_vals)
    args = T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_boost", path])
    v = T.recommend_boost_vector(args, train, I)
    assert v.dtype == np.float32 and np.array_equal(v, file_vals)
    args = T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_novelty", "0.25"])
    v = T.recommend_boost_vector(args, train, I)
    assert v.dtype == np.float32 and np.array_equal(v, np.float32(0.25) * info)
    assert v[1] < v[4] < v[0]                                                   # the more positives, the smaller the weight
    args = T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_novelty", "0.25", "--recommend_boost", path])
    v = T.recommend_boost_vector(args, train, I)
    assert v.dtype == np.float32 and np.array_equal(v, file_vals + np.float32(0.25) * info)
    np.save(path, np.zeros(I + 1, np.float32))
    with pytest.raises(ValueError):
        T.recommend_boost_vector(args, train, I)

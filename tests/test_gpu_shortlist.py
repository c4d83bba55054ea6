"""GPU tests of the bf16 shortlist index (tlsan_shortlist_build / _topk / _select, ShortlistIndex, recommend's index= with
shortlist= and fallback=) against tests/shortlist_ref.py and against the exact path itself: the snapshot's bits, stage 1's
shortlists within the derived fp32 tolerance, and the promise -- a certified row IS recommend()'s row without an index, ids
and score bits, and with the fallback every row is.

Two mutants these tests catch: a certificate without its eps term (s_K > a~_N alone) certifies the rounding counter-example
and returns A where the exact answer is O (test_rounding_counter_example), and certifies tied rows
(test_crowded_rows_do_not_certify); a stage 1 that breaks ties of the approximate
score towards the HIGHER id puts O inside that example's shortlist and drops a B, which the same test's id check catches,
and fails test_crowded's lists (all scores tie: the shortlist must be ids 0 .. N - 1)."""
import ctypes as C

import numpy as np
import pytest

from tests import shortlist_ref as sref
from tests.helpers import batch_tuple, bits, host, make_config, model, p32, random_batch, random_params

pytestmark = pytest.mark.gpu

DS = (64, 128, 256)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def _ws(n):
    import torch
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gauss(n, d, seed, s=1.0):
    return (np.random.RandomState(seed).randn(n, d) * s).astype(np.float32)


def _index_of(w):
    """a ShortlistIndex from the reference's rounding of w (stage 1 alone: the build is tested by itself)"""
    import torch
    from tlsan_amd.shortlist import ShortlistIndex
    vec = _dev(sref.bf16_bits(w).view(np.int16)).view(torch.bfloat16)
    return ShortlistIndex(vec, _dev(np.float32([sref.wmax(w)])))


def _csr(sets, B):
    off = np.zeros(B + 1, np.int32)
    ids = []
    for r in range(B):
        x = sorted(sets[r])
        ids += x
        off[r + 1] = len(ids)
    return _dev(off), _dev(np.asarray(ids + [0], np.int32))


def _stage1(index, ut, N, P=None, bias=None, excl=(None, None), id_mul=1, id_add=0):
    from tlsan_amd import _lib as L, shortlist
    scale = None if P is None else _dev(np.float32([P]))
    b = _dev(bias)
    utd = _dev(ut)
    ids, approx = shortlist.stage1(L.load(), index, utd, ut.shape[0], N, excl, None if scale is None else scale.data_ptr(),
                                   b.data_ptr(), 1, id_mul, id_add, _ws, _stream())
    return host(ids).astype(np.int64), host(approx)


# ---- 1. the snapshot
@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", DS)
def test_build(d, table_dtype):
    for I in (1, 257, 4099):
        cfg = make_config(U=20, I=I, C=5, d=d, H=8)
        _, cat = random_batch(cfg, B=4, Sn=2, seed=d + I)
        p = p32(random_params(cfg, seed=I))
        p["item_emb"] = _gauss(I, d // 2, 3 * I + 1, 0.6).astype(np.float64)
        m = model(cfg, cat, p, table_dtype=table_dtype)
        w = np.concatenate([host(m.item_emb.float()), host(m.cate_emb.float())[cat]], 1)      # the values as stored
        a, b = m.shortlist_index(), m.shortlist_index()
        got = host(a.vec.view(__import__("torch").int16)).view(np.uint16)
        assert got.shape == (I, d) and np.array_equal(got, sref.bf16_bits(w)), (d, I, table_dtype)
        want = sref.wmax(w)
        assert abs(float(host(a.wmax)[0]) - want) <= 2.0 ** -20 * want, (d, I, float(host(a.wmax)[0]), want)
        assert np.array_equal(bits(host(a.wmax)), bits(host(b.wmax)))   # the same table: the same bits
        assert np.array_equal(host(b.vec.view(__import__("torch").int16)), host(a.vec.view(__import__("torch").int16)))
    if table_dtype == "f32":
        e = host(m.item_emb).copy()
        e[I // 2, 3] = np.inf
        _put(m, "item_emb", e)
        assert not np.isfinite(host(m.shortlist_index().wmax)[0])


# ---- 2. stage 1 alone
def _stage1_reference(d, ut, w, bias, P, N, sets, I, id_mul=1, id_add=0):
    """The reference of one case for all rows of ut, and nothing of the GPU: approx / tol [B, I], the eligible pairs, the
    shortlists (local ids) and, per row, the entries that are "unsure": within the tolerance of the reference's N-th score
    -- |a~_ref(j) - a~_ref(N-th)| <= tol(j), with the N-th entry itself once it has such a neighbour.  sets: the rows' excluded
    GLOBAL ids."""
    B = ut.shape[0]
    approx, absprod = sref.approx_scores(ut, w[:I], 1.0 if P is None else P, bias[:I])
    tol = sref.stage1_tolerance(d, 1.0 if P is None else P, absprod, approx)
    glob = np.arange(I) * id_mul + id_add
    ok = np.ones((B, I), bool)
    if sets is not None:
        for r in range(B):
            ok[r] = ~np.isin(glob, list(sets[r]))
    rid, _ = sref.shortlist(approx, ok, N)                               # local ids; the order is the global ids' (monotone)
    unsure = np.zeros((B, I), bool)
    for r in range(B):
        if rid[r, N - 1] >= 0:
            last = rid[r, N - 1]
            near = ok[r] & (np.abs(approx[r] - approx[r, last]) <= tol[r])
            near[last] = False
            if near.any():
                unsure[r] = near
                unsure[r, last] = True
    return dict(approx=approx, tol=tol, ok=ok, rid=rid, unsure=unsure, I=I, N=N, id_mul=id_mul, id_add=id_add)


def _unsure_share(ref, B):
    """(unsure entries, entries) of the reference's shortlists of the first B rows"""
    n = un = 0
    for r in range(B):
        want = ref["rid"][r][ref["rid"][r] >= 0]
        un += int(ref["unsure"][r, want].sum())
        n += len(want)
    return un, n


def _check_stage1(ref, gid, gap):
    """gid / gap [B, N] of a launch over the first B rows of the reference's case"""
    approx, tol, ok, I, N, id_mul, id_add = (ref[k] for k in ("approx", "tol", "ok", "I", "N", "id_mul", "id_add"))
    for r in range(gid.shape[0]):
        want = ref["rid"][r][ref["rid"][r] >= 0]
        n = len(want)
        assert n == min(N, int(ok[r].sum()))
        g = gid[r]
        assert (g[n:] == -1).all() and np.isneginf(gap[r, n:]).all() and (g[:n] >= 0).all(), (r, n)
        loc = (g[:n] - id_add) // id_mul
        assert ((loc * id_mul + id_add) == g[:n]).all() and (loc < I).all() and ok[r, loc].all() and len(set(loc.tolist())) == n
        assert (np.abs(gap[r, :n].astype(np.float64) - approx[r, loc]) <= tol[r, loc]).all(), (r, np.abs(gap[r, :n] - approx[r, loc]).max())
        key = list(zip((-(gap[r, :n] + np.float32(0.0))).tolist(), g[:n].tolist()))
        assert key == sorted(key), r                                     # the launch's own order: score, then the lower id
        unsure = ref["unsure"][r]
        a, b = set(want[~unsure[want]].tolist()), set(loc[~unsure[loc]].tolist())
        assert a == b, (r, sorted(a ^ b))


@pytest.mark.parametrize("d", DS)
def test_stage1_matches_the_reference(d):
    from tlsan_amd import _lib as L
    IMAX, BMAX = 4099, 70
    w = _gauss(IMAX, d, 10 + d, 0.5)
    ut = _gauss(BMAX, d, 20 + d, 1.3)
    bias = np.random.RandomState(30 + d).uniform(-0.3, 0.3, IMAX).astype(np.float32)
    rng = np.random.RandomState(40 + d)
    lib = L.load()
    assert lib.tlsan_shortlist_workspace_bytes(257, 17, d, 64) > 256 >= lib.tlsan_shortlist_workspace_bytes(15, 17, d, 64)   # item slices
    # the cases and their references, each computed once for all rows (a row's shortlist does not depend on B)
    cases = []
    for I in (15, 257, 4099):
        sets = [set(rng.randint(0, I, 12).tolist()) | {int(np.argmax(w[:I] @ ut[r]))} for r in range(BMAX)]
        for N in (16, 64, 256):
            for P, excl in ((0.8125, None), (None, sets)):
                cases.append((I, N, (1, 17, 40, 70) if I == 4099 else (1, 17, 40), P, excl, 1, 0))
    # the item-sharded form: local item n is global id 2 n + 1; the exclusion lists hold global ids
    sets = [set((2 * rng.randint(0, 257, 12) + 1).tolist()) | set((2 * rng.randint(0, 257, 5)).tolist()) for _ in range(BMAX)]
    cases.append((257, 64, (40,), 0.8125, sets, 2, 1))
    refs = [_stage1_reference(d, ut[:max(Bs)], w, bias, P, N, excl, I, id_mul, id_add) for I, N, Bs, P, excl, id_mul, id_add in cases]
    # first the reference alone: few entries are excused on these inputs
    un = n = 0
    for ref, case in zip(refs, cases):
        for B in case[2]:
            a, b = _unsure_share(ref, B)
            un, n = un + a, n + b
    assert n > 0 and un <= 0.01 * n, (un, n)
    # then the launches
    index = {I: _index_of(w[:I]) for I in (15, 257, 4099)}
    for ref, (I, N, Bs, P, excl, id_mul, id_add) in zip(refs, cases):
        for B in Bs:
            gid, gap = _stage1(index[I], ut[:B], N, P=P, bias=bias[:I], excl=(None, None) if excl is None else _csr(excl, B),
                               id_mul=id_mul, id_add=id_add)
            _check_stage1(ref, gid, gap)


# ---- the model-level cases
def _gauss_model(d, I, seed, lazy=False, B=40, cat=None, **kw):
    """a model with Gaussian item / category tables and trained-like biases; lazy: two lazy-L2 steps, so P != 1"""
    cfg = make_config(U=120, I=I, C=23, d=d, H=8)
    b, rcat = random_batch(cfg, B=B, Sn=3, seed=seed + 1, test=True)
    cat = rcat if cat is None else cat
    p = random_params(cfg, seed=seed)
    rng = np.random.RandomState(seed + 2)
    p["item_emb"] = rng.randn(*p["item_emb"].shape) * 0.3
    p["cate_emb"] = rng.randn(*p["cate_emb"].shape) * 0.3
    p["item_b"] = rng.randn(*p["item_b"].shape) * 0.2
    m = model(cfg, cat, p32(p), l2_mode="lazy" if lazy else "dense", **kw)
    if lazy:
        tb, _ = random_batch(cfg, B=64, Sn=3, seed=seed + 3)
        for _ in range(2):
            m.train(None, batch_tuple(tb), 1.0)
        assert m.table_scale() != 1.0
    return cfg, m, b


def _put(m, name, a):
    """overwrite one table of a model in place (its stored values; the state is untouched)"""
    import torch
    t = getattr(m, name)
    t.copy_(torch.as_tensor(np.asarray(a, np.float32)).reshape(t.shape))


def _same(got, want, rows=None):
    g, w = [host(t) for t in got], [host(t) for t in want]
    if rows is not None:
        g, w = [x[rows] for x in g], [x[rows] for x in w]
    return np.array_equal(g[0], w[0]) and np.array_equal(bits(g[1]), bits(w[1]))


# ---- 3. soundness
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("d", DS)
def test_certified_rows_are_the_exact_rows(d, lazy):
    cfg, m, b = _gauss_model(d, 4099, 100 + d, lazy=lazy)
    tup = batch_tuple(b, True)
    index = m.shortlist_index()
    seen = 0
    for kw in ({}, dict(exclude="history")):
        exact = m.recommend(tup, 10, **kw)
        for N in (None, 32, 256):
            raw = m.recommend(tup, 10, index=index, shortlist=N, fallback=False, **kw)
            cert = host(index.certified)
            assert cert.dtype == np.bool_ and cert.shape == (40,)
            assert _same(raw, exact, rows=cert), (d, lazy, N, list(kw))
            seen += int(cert.sum())
            assert _same(m.recommend(tup, 10, index=index, shortlist=N, **kw), exact), (d, lazy, N, list(kw))
            assert np.array_equal(host(index.certified), cert)
    rows, certified = index.counts
    assert rows == 2 * 3 * 2 * 40 and certified == 2 * seen and seen > 0


# ---- 4. a planted gap: every row must certify
def test_planted_gap_certifies_every_row():
    d, I, K, N = 128, 4099, 10, 64
    cfg, m, b = _gauss_model(d, I, 300)
    tup = batch_tuple(b, True)
    sc = host(m.score_candidates(tup, np.tile(np.arange(I), (40, 1))))
    _, _, ut, _ = m.forward(tup, is_test=True, want_u_t=True)
    ut = host(ut)
    w = np.concatenate([host(m.item_emb), host(m.cate_emb)[host(m.item_cate)]], 1)
    wm = sref.wmax(w)
    planted = np.random.RandomState(7).choice(I, K, replace=False)
    bound = sref.epsilon(ut, 1.0, wm, np.abs(sc).max() * 4, np.abs(sc).max() * 4).max()
    item_b = host(m.item_b).copy()
    item_b[planted] += np.float32((sc.max() - sc.min()) + 10.0 * bound)
    _put(m, "item_b", item_b)
    sc = host(m.score_candidates(tup, np.tile(np.arange(I), (40, 1))))
    approx, _ = sref.approx_scores(ut, w, 1.0, item_b)
    ids, _, cert, eps, gap = sref.certify(sc, approx, np.ones((40, I), bool), N, K, ut, 1.0, wm)
    assert (gap >= 8.0 * eps).all() and cert.all()                       # the reference alone: the gap is there
    assert (np.sort(ids, 1) == np.sort(planted)[None, :]).all()
    index = m.shortlist_index()
    got = m.recommend(tup, K, index=index, shortlist=N, fallback=False)
    assert host(index.certified).all()
    assert _same(got, m.recommend(tup, K)) and np.array_equal(host(got[0]), ids)


# ---- 5. crowded: all scores tie
def test_crowded_rows_do_not_certify():
    d, I, K, N = 64, 300, 10, 64
    cfg, m, b = _gauss_model(d, I, 400, cat=np.zeros(300, np.int32))
    e = host(m.item_emb).copy()
    e[:] = e[0]
    _put(m, "item_emb", e)
    _put(m, "item_b", np.full(I, 0.125, np.float32))
    tup = batch_tuple(b, True)
    index = m.shortlist_index()
    exclude = [[] for _ in range(40)]
    exclude[3] = list(range(20, I))                                       # 20 eligible items: fewer than N
    exclude[11] = list(range(0, I - 63))                                  # 63
    exclude[12] = list(range(0, I - 64))                                  # 64: a full shortlist
    raw = m.recommend(tup, K, index=index, shortlist=N, fallback=False, exclude=exclude)
    cert = host(index.certified)
    assert cert[3] and cert[11] and cert.sum() == 2
    got = m.recommend(tup, K, index=index, shortlist=N, exclude=exclude)
    assert _same(got, m.recommend(tup, K, exclude=exclude))
    ids = host(got[0])
    assert np.array_equal(ids[0], np.arange(K)) and np.array_equal(ids[3], np.arange(K)) and np.array_equal(ids[12], np.arange(I - 64, I - 64 + K))
    assert _same(raw, got)                                               # (ties to the lower id in both stages: the same lists here)
    plain = m.recommend(tup, K, index=index, shortlist=N, fallback=False)
    assert not host(index.certified).any() and np.array_equal(host(plain[0]), np.tile(np.arange(K), (40, 1)))


# ---- 6. / 7. rows given as u_t: the rounding counter-example, a NaN row
def _lists_of(m, ut, K, N, index, fallback):
    from tlsan_amd import shortlist
    return shortlist.shortlist_topk(m.lib, m.dims, m.cparams, ut, int(ut.shape[0]), K, (None, None), index, N, fallback,
                                    m._topk_workspace, m._stream())


def test_rounding_counter_example():
    """tests/test_shortlist_cpu.py has the numbers; here the kernels run them: O ties B in bf16 and falls outside the shortlist
    of 16, its exact score beats A's, and the row does not certify because the gap 0.0078 is below eps = 0.012."""
    d, N, K = 64, 16, 1
    ut, w = sref.counter_example(d, N)
    cfg = make_config(U=20, I=N + 1, C=1, d=d, H=8)
    _, cat = random_batch(cfg, B=4, Sn=2, seed=1)
    p = p32(random_params(cfg, seed=2))
    p["item_emb"], p["cate_emb"], p["item_b"] = w[:, :d // 2], np.zeros((1, d // 2)), np.zeros(N + 1)
    m = model(cfg, cat, p)
    index = m.shortlist_index()
    assert np.array_equal(host(index.vec.float()), sref.bf16_round(w))
    utd = _dev(ut)
    sid, sap = _stage1(index, ut, N, bias=np.zeros(N + 1, np.float32))
    assert sorted(sid[0].tolist()) == list(range(N)) and sap[0, N - 1] == np.float32(1.0 + 2.0 ** -6)   # O is outside
    raw = _lists_of(m, utd, K, N, index, False)
    assert not host(index.certified)[0] and host(raw[0])[0, 0] == 0      # A leads the shortlist, and the row says it is unsure
    got = _lists_of(m, utd, K, N, index, True)
    from tlsan_amd.model import eval_topk
    want = eval_topk(m.lib, m.dims, m.cparams, utd, 1, K, (None, None), 1, 0, m._topk_workspace, m._stream())
    assert host(got[0])[0, 0] == N and _same(got, want)                  # the fallback returns O


def test_nan_row_is_not_certified():
    from tlsan_amd.model import eval_topk
    cfg, m, b = _gauss_model(128, 4099, 500)
    tup = batch_tuple(b, True)
    _, _, ut, _ = m.forward(tup, is_test=True, want_u_t=True)
    index = m.shortlist_index()
    _lists_of(m, ut, 10, 64, index, False)
    clean = host(index.certified)
    bad = ut.clone()
    bad[5] = float("nan")
    bad[22, 7] = float("inf")
    raw = _lists_of(m, bad, 10, 64, index, False)
    cert = host(index.certified)
    others = np.ones(40, bool)
    others[[5, 22]] = False
    assert not cert[5] and not cert[22] and np.array_equal(cert[others], clean[others]) and clean[others].any()
    want = eval_topk(m.lib, m.dims, m.cparams, bad, 40, 10, (None, None), 1, 0, m._topk_workspace, m._stream())
    assert _same(raw, want, rows=cert)
    assert _same(_lists_of(m, bad, 10, 64, index, True), want)


# ---- 8. composition and the refusals
def test_composition_and_value_errors():
    cfg, m, b = _gauss_model(128, 1500, 600)
    tup = batch_tuple(b, True)
    index = m.shortlist_index()
    for kw in (dict(diversity=0.3), dict(per_category=2), dict(diversity=0.5, per_category=1, pool=40, exclude="history")):
        assert _same(m.recommend(tup, 10, index=index, **kw), m.recommend(tup, 10, **kw)), list(kw)
    assert index.certified.shape == (40,)
    other = _gauss_model(64, 1500, 601)[1].shortlist_index()
    before = index.counts
    for kw in (dict(within=m.item_scope(items=np.arange(0, 1500, 3))), dict(category=np.zeros(40, np.int64)), dict(probes=4),
               dict(shortlist=10), dict(shortlist=15), dict(shortlist=300), dict(pool=64, diversity=0.2, shortlist=64)):
        with pytest.raises(ValueError):
            m.recommend(tup, 10, index=index, **kw)
    with pytest.raises(ValueError):
        m.recommend(tup, 10, index=other)                                # another d
    with pytest.raises(ValueError):
        m.recommend(tup, 10, shortlist=64)                               # shortlist= without the index
    assert index.counts == before                                        # refused before any launch


# ---- 9. the driver
def test_driver_serves_the_same_lists_and_counts_real_rows(tmp_path):
    """train.py --shortlist_index 1 writes the file the plain run writes, bit for bit, and reports the certified share over
    the test set's rows (not over the rows that pad a launch)."""
    import os
    from tlsan_amd import train as T
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    common = ["--dataset", ds, "--max_steps", "5", "--eval_freq", "1000", "--quiet", "--eval_topk", "0", "--seed", "7", "--recommend_k", "10"]
    plain = T.train(T.parse(common + ["--model_dir", str(tmp_path / "a")]))
    short = T.train(T.parse(common + ["--model_dir", str(tmp_path / "b"), "--shortlist_index", "1", "--shortlist", "32"]))
    a, b = np.load(T.recommend_path(str(tmp_path / "a"), 10)), np.load(T.recommend_path(str(tmp_path / "b"), 10))
    assert np.array_equal(a["user"], b["user"]) and np.array_equal(a["ids"], b["ids"])
    assert np.array_equal(bits(a["scores"]), bits(b["scores"]))
    rows, cert = short["shortlist_certified"]
    assert rows == len(a["user"]) and 0 <= cert <= rows and "shortlist_certified" not in plain

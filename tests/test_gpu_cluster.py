"""GPU tests of the clustered item index (tlsan_cluster_assign / _means / _probe, ClusteredIndex, recommend's and
similar_items' index= with probes=) against tests/cluster_ref.py: the three kernels on seeded Gaussians at the tile edges,
the served lists against the exact path (all lists probed: bit for bit) and against the selection of tests/scope_ref.py
over the union of the probed lists (fewer probes), the fit on a planted table against the reference's Lloyd from the same
train_ids / init_ids, and the state.

Two mutants these tests catch: ties in the probe going to the HIGHER list id fail test_probe_ties_empty_lists_and_fill (and
the duplicate centroids' rows of it); means summed in arrival order with floating-point atomics fail test_means (its
64-row segment alternates +-2^60 with small values, so only the order given produces the reference's bits; in float32 the
600-row segment leaves the 1-ulp band as well)."""
import ctypes as C

import numpy as np
import pytest

from tests import cluster_cases as cases, cluster_ref as cref, lists_ref, scope_ref
from tests.helpers import (batch_tuple, bits, history_sets, host, lazy_model, make_config, model, p32, random_batch,
                           random_params, sharded)
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

DS = cases.DS


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")


def _ws(n):
    import torch
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _assign(x, cent, want_dist=True):
    from tlsan_amd import _lib as L, cluster
    a, dist = cluster.cluster_assign(L.load(), _dev(x), _dev(cent), _ws, _stream(), want_dist=want_dist)
    return host(a).astype(np.int64), (host(dist) if want_dist else None)


def _means(x, order, seg, cent):
    from tlsan_amd import _lib as L, cluster
    c = _dev(cent).clone()
    cluster.cluster_means(L.load(), _dev(x), _dev(np.asarray(order, np.int32)), _dev(np.asarray(seg, np.int32)), c, _stream())
    return host(c)


def _probe(q, cent, P, scale=None, bias=None, list_off=None):
    import torch
    from tlsan_amd import _lib as L
    lib = L.load()
    B, d = q.shape
    nc = len(cent)
    ws = _ws(lib.tlsan_cluster_workspace_bytes(B, nc, P))
    rows = torch.full((B, P), -7, dtype=torch.int32, device="cuda:0")
    t = [None if v is None else _dev(np.asarray(v, dt)) for v, dt in ((scale, np.float32), (bias, np.float32), (list_off, np.int32))]
    ptr = lambda v: None if v is None else v.data_ptr()
    qd, cd = _dev(q), _dev(cent)
    L.check(lib.tlsan_cluster_probe(qd.data_ptr(), B, d, cd.data_ptr(), ptr(t[0]), ptr(t[1]), ptr(t[2]), nc, P, rows.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()), "tlsan_cluster_probe")
    return host(rows).astype(np.int64)


_gauss = cases.gauss


# ---- 1. assign
@pytest.mark.parametrize("d", DS)
def test_assign_matches_the_reference_at_the_tile_edges(d):
    for nc in cases.ASSIGN_C:
        x600, cent = cases.assign_case(d, nc)
        want, wdist, sure, err = cref.assign(x600, cent)
        assert (~sure).mean() <= 0.01, (nc, (~sure).mean())            # (the reference alone: few rows are excused)
        full = None
        for N in cases.ASSIGN_N:
            got, dist = _assign(x600[:N], cent)
            ok = sure[:N]
            assert np.array_equal(got[ok], want[:N][ok]), (d, N, nc)
            assert ((got >= 0) & (got < nc)).all()
            assert (np.abs(dist[ok] - wdist[:N][ok]) <= err[:N][ok]).all(), (d, N, nc, np.abs(dist[ok] - wdist[:N][ok]).max())
            # an excused row: the distance to the centroid the kernel chose, within the bound of that centroid's value
            ref_d = np.maximum((x600[:N].astype(np.float64) ** 2).sum(1) - 2.0 * cref.values(x600[:N], cent)[np.arange(N), got], 0.0)
            assert (np.abs(dist - ref_d) <= err[:N]).all(), (d, N, nc)
            if N == 600:
                full = (got, dist)
            else:                                                       # a row's result does not depend on N
                assert np.array_equal(got, full[0][:N]) and np.array_equal(bits(dist), bits(full[1][:N])), (d, N, nc)


def test_assign_duplicates_nan_rows_and_no_dist():
    d = 128
    x = _gauss(600, d, 3)
    cent = _gauss(40, d, 4)
    far = cent.copy()
    far[[5, 33]] = 100.0                                                # (never the nearest: what the duplicates must not win)
    cent[5], cent[33] = cent[2], cent[17]                               # bit-identical rows: equal values -> the lower id
    cent[20] = np.nan                                                   # a NaN centroid is never the best
    far[20] = 100.0
    want, _, sure, _ = cref.assign(x, far)
    assert sure.mean() >= 0.99 and (want == 2).any() and (want == 17).any()
    x[7] = np.nan
    x[300, 5] = np.nan
    got, _ = _assign(x, cent, want_dist=False)
    sure[[7, 300]] = True
    want[[7, 300]] = 0                                                  # a row whose best value is NaN: list 0
    assert np.array_equal(got[sure], want[sure])
    assert not np.isin(got, [5, 33, 20]).any()


# ---- 2. means
@pytest.mark.parametrize("d", DS)
def test_means(d):
    sizes = [0, 1, 17, 600, 0, 3]
    n = sum(sizes) + 5                                                  # (five rows nobody names)
    x = (_gauss(n, d, 11) * 3.0 + 0.5).astype(np.float32)
    order = np.random.RandomState(12).permutation(n)[:sum(sizes)]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    cent0 = _gauss(len(sizes), d, 13)
    want = cref.means(x, order, seg, cent0)
    got = _means(x, order, seg, cent0)
    assert np.array_equal(bits(got[[0, 4]]), bits(cent0[[0, 4]]))       # an empty segment is left untouched
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert np.array_equal(bits(got[1]), bits(x[order[0]]))              # one row: itself
    assert np.array_equal(bits(_means(x, order, seg, cent0)), bits(got))  # a function of the inputs, bit for bit
    # the order given: 64 rows that alternate +-2^60 with small values -- a small value after +2^60 is lost in float64, one
    # after -2^60 is kept, so any other summation order gives another mean (an arrival-order sum fails here whatever its type)
    y = _gauss(64, d, 14)
    y[0::4], y[2::4] = 2.0 ** 60, -2.0 ** 60
    rng = np.random.RandomState(15)
    for c in range(d):                                                  # (another order in every column)
        y[:, c] = y[rng.permutation(16).repeat(4) * 4 + np.tile(np.arange(4), 16), c]
    for perm in (np.arange(64), rng.permutation(64)):
        want = cref.means(y, perm, [0, 64], cent0[:1])
        got = _means(y, perm, [0, 64], cent0[:1])
        assert np.array_equal(bits(got), bits(want)), d
    assert not np.array_equal(bits(cref.means(y, np.arange(64), [0, 64], cent0[:1])), bits(want))


# ---- 3. probe
@pytest.mark.parametrize("d", DS)
def test_probe_matches_the_reference_order(d):
    for name, q, cent, P, kw in cases.probe_cases(d):
        want = cref.probe(q, cent, P, **kw)
        sure = cref.probe_sure(q, cent, P, **kw)
        assert (~sure).mean() <= 0.01, (name, (~sure).mean())          # (the reference alone: few slots are excused)
        got = _probe(q, cent, P, **kw)
        assert np.array_equal(got[sure], want[sure]), name
        live = min(P, cases.live_lists(cent, kw))
        assert (got[:, live:] == -1).all() and (got[:, :live] >= 0).all() and (got < len(cent)).all(), name
        assert all(len(set(r[:live].tolist())) == live for r in got), name                  # no list twice
        if "list_off" in kw:
            assert (np.diff(kw["list_off"])[got[:, :live]] > 0).all(), name                 # empty lists are skipped
        if P == 8:
            assert np.array_equal(_probe(q[:1], cent, P, **kw), got[:1]), name              # a row's lists depend on that row only


def test_probe_ties_empty_lists_and_fill():
    d = 64
    q = _gauss(33, d, 31)
    cent = _gauss(20, d, 32)
    tied = [3, 4, 9, 15]
    cent[tied] = cent[3]                                                # bit-identical centroids
    bias = np.zeros(20, np.float32)
    bias[tied] = 1000.0                                                 # far ahead of the rest
    got = _probe(q, cent, 4, bias=bias)
    assert (got == np.asarray(tied)[None, :]).all()                     # equal scores: the lower list first
    off = np.concatenate([[0], np.cumsum([1] * 20)])
    off[5:] -= 1                                                        # list 4 is empty
    got = _probe(q, cent, 6, bias=bias, list_off=off)
    assert (got[:, :3] == np.asarray([3, 9, 15])[None, :]).all() and not (got == 4).any() and (got[:, 3:] >= 0).all()
    nan_bias = bias.copy()
    nan_bias[0] = np.nan
    got = _probe(q, cent, 64, bias=nan_bias)
    assert (got[:, :4] == np.asarray(tied)[None, :]).all()
    assert (got[:, 19] == 0).all() and (got[:, 20:] == -1).all()        # NaN last, then the fill: C < P
    assert all(sorted(r[:20].tolist()) == list(range(20)) for r in got)


# ---- 4. end to end
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _equal(a, b):
    a, b = [host(t) for t in a], [host(t) for t in b]
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1])


I0, B0 = 600, 48
DIVERSE = dict(diversity=0.3, per_category=2, pool=40)


def _rows(b, n):
    return batch_tuple({k: v[:n] for k, v in b.items()}, True)


def _check_partial(m, b, ci, P, k, sc_all):
    """probes < nlists: the selection of scope_ref from the model's own scores over the union of the probed lists"""
    tup = _rows(b, B0)
    _, _, ut, _ = m.forward(tup, is_test=True, want_u_t=True)
    rl = host(ci.probe(ut, P, scale=m._scale_vector(ci.lists), bias=ci.list_bias))
    off, items = host(ci.partition.list_off), host(ci.partition.list_items)
    for exclude, sets in ((None, None), ("history", history_sets(b))):
        ok = lists_ref.union_mask(B0, I0, rl, off, items, exclude=sets)
        want = scope_ref.topk(sc_all, ok, k)
        got = m.recommend(tup, k, exclude=exclude, index=ci, probes=P)
        assert np.array_equal(host(got[0]), want[0]) and _same(host(got[1]), want[1]), (P, exclude)


@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (128, 4)])
def test_recommend_with_every_list_probed_is_the_exact_path(d, H):
    cfg = make_config(U=60, I=I0, C=9, d=d, H=H)
    b, cat = random_batch(cfg, B=B0, Sn=3, seed=52, test=True)
    m = model(cfg, cat, p32(random_params(cfg, seed=51)))
    sc_all = host(m.score_candidates(_rows(b, B0), np.tile(np.arange(I0), (B0, 1))))
    exact = {}
    for nlists in (5, 8, 12, 24):
        ci = m.cluster_index(nlists, iters=4, seed=nlists)
        assert ci.lists == nlists and ci.count == I0 and sorted(host(ci.partition.list_items)[:I0].tolist()) == list(range(I0))
        for B in (1, 17, B0):
            tup = _rows(b, B)
            for name, kw in (("plain", {}), ("history", dict(exclude="history")), ("diverse", DIVERSE)):
                if (B, name) not in exact:
                    exact[B, name] = m.recommend(tup, 10, **kw)
                assert _equal(m.recommend(tup, 10, index=ci, probes=nlists, **kw), exact[B, name]), (nlists, B, name)
        assert _equal(m.recommend(_rows(b, B0), 10, index=ci, probes=min(64, nlists + 7)), exact[B0, "plain"])
        _check_partial(m, b, ci, max(1, nlists // 3), 10, sc_all)
    ci = m.cluster_index(12, iters=4, seed=3, max_list=20)              # oversized lists cut: more lists, the same items
    assert ci.lists > 12 and ci.max_list <= 20
    assert _equal(m.recommend(_rows(b, B0), 10, index=ci, probes=ci.lists), exact[B0, "plain"])
    _check_partial(m, b, ci, 9, 10, sc_all)
    scope = m.item_scope(items=np.arange(0, I0, 3))                     # the scope belongs to the index
    si = m.cluster_index(8, within=scope, iters=3)
    assert _equal(m.recommend(_rows(b, B0), 10, index=si, probes=8), m.recommend(_rows(b, B0), 10, within=scope))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_similar_items_with_a_clustered_index(metric):
    from tlsan_amd import model as M
    cfg = make_config(U=60, I=I0, C=9, d=128, H=8)
    b, cat = random_batch(cfg, B=B0, Sn=3, seed=52, test=True)
    m = model(cfg, cat, p32(random_params(cfg, seed=53)))
    qids = np.arange(0, I0, 13)
    excl = [[int(q) // 2, 3, 6] for q in qids]
    for nlists in (5, 12, 24):
        ci = m.cluster_index(nlists, iters=4, seed=nlists)
        for exclude in (None, excl):
            for k in (5, 64):
                got = m.similar_items(qids, k, metric=metric, exclude=exclude, index=ci, probes=nlists)
                assert _equal(got, m.similar_items(qids, k, metric=metric, exclude=exclude)), (nlists, k)
        # fewer probes: the exact lists within the union of the probed lists (a scope per query), bit for bit
        P = max(1, nlists // 3)
        v, _ = M.item_vectors(m.lib, m.dims, m.cparams, _dev(qids.astype(np.int32)), 1, 0, m._stream())
        rl = host(ci.probe(v, P, scale=ci.centroid_inv if metric == "cosine" else None))
        off, items = host(ci.partition.list_off), host(ci.partition.list_items)
        got = [host(t) for t in m.similar_items(qids, 7, metric=metric, index=ci, probes=P)]
        for r, q in enumerate(qids):
            mine = np.concatenate([items[off[c]:off[c + 1]] for c in rl[r] if c >= 0])
            want = [host(t) for t in m.similar_items([int(q)], 7, metric=metric, within=m.item_scope(items=mine))]
            assert np.array_equal(got[0][r], want[0][0]) and _same(got[1][r], want[1][0]), (nlists, r)


@pytest.mark.parametrize("table_dtype", ["bf16", "f32"])
def test_lazy_l2_and_bf16_tables(table_dtype):
    cfg, m = lazy_model(I0, table_dtype, seed=41)                       # d = 256, P != 1
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=43, test=True)
    sc_all = host(m.score_candidates(_rows(b, B0), np.tile(np.arange(I0), (B0, 1))))
    ci = m.cluster_index(12, iters=4)
    tup = _rows(b, B0)
    for kw in ({}, dict(exclude="history"), DIVERSE):
        assert _equal(m.recommend(tup, 10, index=ci, probes=12, **kw), m.recommend(tup, 10, **kw)), list(kw)
    _check_partial(m, b, ci, 3, 10, sc_all)
    qids = np.arange(0, I0, 37)
    for metric in ("cosine", "dot"):
        assert _equal(m.similar_items(qids, 10, metric=metric, index=ci, probes=12), m.similar_items(qids, 10, metric=metric))


# ---- 5. fit
def _planted_model():
    """tests/cluster_cases.py's planted table as a model's item and category tables"""
    vec, item_half, cate_rows, lab = cases.planted_table()
    cfg = make_config(U=60, I=I0, C=12, d=cases.PLANTED_D, H=8)
    p = p32(random_params(cfg, seed=61))
    p["item_emb"], p["cate_emb"] = item_half.astype(np.float64), cate_rows.astype(np.float64)
    b, _ = random_batch(cfg, B=B0, Sn=3, seed=62, test=True)
    return cfg, model(cfg, lab.astype(np.int32), p), b, vec


def _tensors(ci):
    return [host(t) for t in (ci.centroids, ci.list_bias, ci.centroid_inv, ci.parent, ci.partition.list_off, ci.partition.list_items)]


def test_fit_on_planted_clusters_equals_the_reference():
    from tlsan_amd import model as M
    from tlsan_amd.cluster import recall
    cfg, m, b, table = _planted_model()
    ci = m.cluster_index(12, iters=10, seed=cases.FIT_SEED)
    train, init = cases.fit_draws(I0, 12, cases.FIT_SEED)
    assert np.array_equal(ci.train_ids, train) and np.array_equal(ci.init_ids, init)
    vec = host(M.item_vectors(m.lib, m.dims, m.cparams, _dev(np.arange(I0, dtype=np.int32)), 1, 0, m._stream())[0])
    assert np.array_equal(bits(vec), bits(table))                       # the vectors are the tables as stored
    cent, _, objective, margin = cref.fit(vec, np.searchsorted(ci.train_ids, ci.init_ids), 10)
    assert margin > 10.0                                                # (the reference alone: no assignment near the bound)
    want, _, sure, _ = cref.assign(vec, cent)
    assert sure.all()
    off, items = lists_ref.index_of(want, 12)
    assert np.array_equal(host(ci.partition.list_off), off) and np.array_equal(host(ci.partition.list_items)[:I0], items)
    # (a row's dist errs by at most the bound, here below 2e-4 of it: 2 (d + 2) 2^-24 (|x| |c| + |c|^2 / 2) against |x - c|^2)
    assert len(ci.objective) == len(objective) and np.allclose(ci.objective, objective, rtol=2e-4, atol=0)
    assert all(z <= a * (1 + 1e-6) for a, z in zip(ci.objective, ci.objective[1:]))
    assert (np.abs(host(ci.centroids).astype(np.float64) - cent) <= np.spacing(np.abs(cent))).all()
    # recall against the exact lists: the library's equals the reference's at every probe count
    tup = _rows(b, B0)
    exact = host(m.recommend(tup, 10)[0])
    sc_all = host(m.score_candidates(tup, np.tile(np.arange(I0), (B0, 1))))
    _, _, ut, _ = m.forward(tup, is_test=True, want_u_t=True)
    bias = np.array([host(m.item_b)[items[off[c]:off[c + 1]]].astype(np.float64).mean() if off[c + 1] > off[c] else 0.0
                     for c in range(12)]).astype(np.float32)
    assert (np.abs(host(ci.list_bias).astype(np.float64) - bias) <= np.spacing(np.abs(bias))).all()
    cent, bias = host(ci.centroids), host(ci.list_bias)                 # (the probe's own operands from here on)
    last = 0.0
    for P in (1, 2, 4, 8, 12):
        assert cref.probe_sure(host(ut), cent, P, bias=bias, list_off=off).all()
        rl = cref.probe(host(ut), cent, P, bias=bias, list_off=off)
        want_ids = scope_ref.topk(sc_all, lists_ref.union_mask(B0, I0, rl, off, items), 10)[0]
        got = host(m.recommend(tup, 10, index=ci, probes=P)[0])
        r = recall(got, exact)
        assert r == cref.recall(want_ids, exact) == cref.recall(got, exact), P
        assert r >= last
        last = r
    assert last == 1.0
    # two builds with one seed: every tensor byte for byte; another seed differs
    again = m.cluster_index(12, iters=10, seed=cases.FIT_SEED)
    assert all(a.tobytes() == z.tobytes() for a, z in zip(_tensors(ci), _tensors(again))) and again.objective == ci.objective
    assert np.array_equal(again.init_ids, ci.init_ids)
    other = m.cluster_index(12, iters=10, seed=99)
    assert not np.array_equal(other.init_ids, ci.init_ids)
    assert any(a.tobytes() != z.tobytes() for a, z in zip(_tensors(ci), _tensors(other)))


# ---- 6. state and arguments
def test_state_is_read_not_changed_and_bad_arguments_are_refused():
    import torch
    cfg = make_config(U=40, I=500, C=7, d=128, H=8)
    tb, cat = random_batch(cfg, B=64, Sn=3, seed=72)
    b, _ = random_batch(cfg, B=30, Sn=3, seed=73, test=True)
    m = model(cfg, cat, random_params(cfg, seed=71), l2_mode="lazy")
    for _ in range(3):
        m.train(None, batch_tuple(tb), 1.0)
    tup = batch_tuple(b, True)
    m.recommend(tup, 5)                                                 # (what the last step owed lands with the first call)
    P = m.table_scale()
    assert P != 1.0
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.cate_emb, m.item_b, m.dense, m.user_emb, m.usert_emb)]
    before = snap()
    ci = m.cluster_index(9, iters=5)
    m.recommend(tup, 20, index=ci, probes=3, exclude="history")
    m.recommend(tup, 5, index=ci, probes=9, per_category=1, diversity=0.5)
    m.similar_items(np.arange(0, 500, 23), 10, index=ci, probes=2)
    m.similar_items(np.arange(0, 500, 23), 10, metric="dot", index=ci, probes=9)
    after = snap()
    assert m.table_scale() == P
    same = lambda xs, ys: all(torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(xs, ys))
    assert same(before, after)
    other = model(make_config(U=40, I=400, C=7, d=128, H=8), cat[:400]).cluster_index(4, iters=1)
    scope = m.item_scope(items=[1, 2, 3])
    for kw in (dict(index=ci), dict(index=ci, probes=0), dict(index=ci, probes=65), dict(index=ci, probes=2.5), dict(probes=3),
               dict(index=m.category_index(), probes=3, category=np.zeros(30, np.int64)), dict(index=other, probes=2),
               dict(index=ci, probes=2, within=scope), dict(index=ci, probes=2, category=np.zeros(30, np.int64))):
        with pytest.raises(ValueError):
            m.recommend(tup, 5, **kw)
    for kw in (dict(index=ci), dict(index=ci, probes=65), dict(probes=3), dict(index=other, probes=2),
               dict(index=ci, probes=2, within=scope), dict(index=ci, probes=2, same_category=True)):
        with pytest.raises(ValueError):
            m.similar_items([1, 2], 5, **kw)
    for bad in (dict(nlists=0), dict(nlists=20000), dict(nlists=4, iters=-1), dict(nlists=600), dict(nlists=4, train_size=3),
                dict(nlists=4, max_list=0), dict(nlists=4, within=[1, 2])):
        with pytest.raises(ValueError):
            m.cluster_index(**bad)
    assert same(before, snap())


def _sharded_refusal(rank, world):
    from tlsan_amd.model import Model
    cfg = make_config(U=30, I=257, C=6, d=128)
    b, cat = random_batch(cfg, B=8, Sn=3, seed=82, test=True)
    sm = sharded(cfg, cat, random_params(cfg, seed=81), l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    ci = m.cluster_index(4, iters=2)
    tup = batch_tuple(b, True)
    for kw in (dict(index=ci, probes=2), dict(index=ci), dict(probes=2)):
        with pytest.raises(ValueError, match="ClusteredIndex"):
            sm.recommend(tup, 5, **kw)
        with pytest.raises(ValueError, match="ClusteredIndex"):
            sm.similar_items([1, 2], 5, **kw)
    with pytest.raises(ValueError, match="ClusteredIndex"):
        sm.cluster_index(4)
    assert sm.recommend(tup, 5)[0].shape == (8, 5)                      # (and the model still serves)


def test_sharded_model_refuses_a_clustered_index():
    run_ranks(_sharded_refusal, 1)


# ---- 7. the driver
def test_driver_writes_the_exact_lists_when_every_list_is_probed(tmp_path):
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ds = os.path.join(root, "tests", "golden", "packed_clothing.npz")
    files, logs = [], []
    for flags in ((), ("--cluster_index", "16", "--cluster_probes", "16", "--recommend_metrics", "1")):
        out = str(tmp_path / ("model%d" % len(files)))
        r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "30",
                            "--eval_freq", "1000", "--recommend_k", "10", "--recommend_exclude", "history"] + list(flags),
                           cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        files.append(np.load(os.path.join(out, "recommend_top10.npz")))
        logs.append(r.stdout)
    assert sorted(files[0].files) == sorted(files[1].files)
    for key in files[0].files:
        a, z = files[0][key], files[1][key]
        assert a.dtype == z.dtype and a.shape == z.shape and a.tobytes() == z.tobytes(), key
    m = re.search(r"Clustered index: recall@10 = ([0-9.]+) against the exact lists over (\d+) rows \(16 probes\)", logs[1])
    assert m and float(m.group(1)) == 1.0 and int(m.group(2)) > 0, logs[1][-1500:]
    assert re.search(r"Clustered index: 16 lists over \d+ items, max / mean list \d+ / [0-9.]+, \d+ k-means iterations", logs[1])
    assert "Clustered index" not in logs[0]

"""CPU tests of the bf16 shortlist index: the numpy reference's own properties (tests/shortlist_ref.py: the rounding, the
error bound the certificate rests on, the rounding counter-example of the certificate's eps term), the header == exports ==
bindings of the four entry points at ABI 15, every refusal of the C ABI (raised on the host, before any launch) and the
ValueErrors of recommend's arguments.  No GPU is touched.

The first four tests (the rounding, the bound, the certificate on Gaussians and on ties, the numpy counter-example) exercise
tests/shortlist_ref.py alone: they hold whatever the library does, and are here because every GPU test leans on that
reference.  The tests that need the feature are the others -- exports, refusals, ValueErrors, the sharded refusal and the
driver's flags -- and tests/test_gpu_shortlist.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import shortlist_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000      # a pointer that is never dereferenced: every call below is refused before any launch


def test_bf16_rounding_is_nearest_even():
    import torch
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.randn(4000).astype(np.float32) * 3.0, rng.randn(100).astype(np.float32) * 1e-30,
                        np.float32([0.0, -0.0, np.inf, -np.inf, 1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                                    3.3895314e38])])
    want = torch.as_tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(sref.bf16_bits(x), want)
    assert sref.bf16_round(np.float32([1.0 + 2.0 ** -8]))[0] == 1.0                       # a tie goes to the even pattern
    assert sref.bf16_round(np.float32([1.0 + 2.0 ** -7 + 2.0 ** -8]))[0] == 1.0 + 2.0 ** -6
    assert np.isnan(sref.bf16_round(np.float32([np.nan]))[0])
    once = sref.bf16_round(x)
    assert np.array_equal(sref.bf16_bits(once), sref.bf16_bits(x))                        # a bf16 value is not rounded twice


@pytest.mark.parametrize("d", [64, 128, 256])
def test_the_bound_holds_for_every_pair(d):
    rng = np.random.RandomState(d)
    for P in (1.0, 0.8125):
        ut = (rng.randn(48, d) * 1.7).astype(np.float32)
        w = (rng.randn(3000, d) * 0.4).astype(np.float32)
        bias = rng.uniform(-0.3, 0.3, 3000).astype(np.float32)
        approx, _ = sref.approx_scores(ut, w, P, bias)
        exact = (ut.astype(np.float64) @ w.astype(np.float64).T) * P + bias.astype(np.float64)[None, :]
        norm = np.sqrt((ut.astype(np.float64) ** 2).sum(1))
        bound = sref.C * abs(P) * norm[:, None] * sref.wmax(w)
        assert (np.abs(approx - exact) <= bound).all()
        assert np.abs(approx - exact).max() > 0.0


def test_the_certificate_on_gaussians_and_on_ties():
    rng = np.random.RandomState(5)
    B, I, d, N, K = 24, 3000, 64, 64, 10
    ut = rng.randn(B, d).astype(np.float32)
    w = (rng.randn(I, d) * 0.3).astype(np.float32)
    bias = rng.uniform(-0.3, 0.3, I).astype(np.float32)
    exact = ((ut.astype(np.float64) @ w.astype(np.float64).T) + bias[None, :]).astype(np.float32)
    approx, _ = sref.approx_scores(ut, w, 1.0, bias)
    ok = np.ones((B, I), bool)
    ok[3, 40:] = False                                                  # a row with fewer than N eligible items
    ids, sc, cert, eps, gap = sref.certify(exact, approx, ok, N, K, ut, 1.0, sref.wmax(w))
    from tests import scope_ref
    want = scope_ref.topk(exact, ok, K)
    assert cert[3] and cert.mean() > 0.5
    assert np.array_equal(ids[cert], want[0][cert]) and np.array_equal(sc[cert], want[1][cert])   # sound
    assert (gap[cert & (np.arange(B) != 3)] > eps[cert & (np.arange(B) != 3)]).all()
    # all scores tie: nothing certifies, whatever the ids say
    w[:] = w[0]
    bias[:] = 0.25
    exact = ((ut.astype(np.float64) @ w.astype(np.float64).T) + bias[None, :]).astype(np.float32)
    approx, _ = sref.approx_scores(ut, w, 1.0, bias)
    _, _, cert, _, _ = sref.certify(exact, approx, ok, N, K, ut, 1.0, sref.wmax(w))
    assert cert[3] and not cert[np.arange(B) != 3].any()
    # non-finite: a NaN row, an infinite norm bound
    ut[5] = np.nan
    _, _, cert, _, _ = sref.certify(exact, approx, ok, N, K, ut, 1.0, np.inf)
    assert cert[3] and cert.sum() == 1


@pytest.mark.parametrize("N", [2, 16])
def test_rounding_counter_example(N):
    """O's approximate score ties B's, O's id is the highest, so O is the one item outside the shortlist; its exact score
    1.023512 beats A's 1.0234375.  The gap s_K - a~_N = 0.0078 is below eps = 0.012: the row must not certify -- and a
    certificate without its eps term certifies it, and would return A where the exact answer is O."""
    from tests import scope_ref
    d, K = 64, 1
    ut, w = sref.counter_example(d, N)
    I = N + 1
    bias = np.zeros(I, np.float32)
    approx, _ = sref.approx_scores(ut, w, 1.0, bias)
    exact = (ut.astype(np.float64) @ w.astype(np.float64).T).astype(np.float32)           # (every product and sum is exact in fp32)
    assert approx[0, N] == approx[0, 1] == 1.0 + 2.0 ** -6 and approx[0, 0] == 1.0 + 2.0 ** -6 + 2.0 ** -7
    assert abs(float(exact[0, N]) - 1.023512) < 1e-6 and exact[0, 0] == np.float32(1.0234375) and exact[0, N] > exact[0, 0]
    ok = np.ones((1, I), bool)
    sid, _ = sref.shortlist(approx, ok, N)
    assert sorted(sid[0].tolist()) == list(range(N))                     # O (id N) fell outside
    ids, sc, cert, eps, gap = sref.certify(exact, approx, ok, N, K, ut, 1.0, sref.wmax(w))
    assert ids[0, 0] == 0 and not cert[0]
    assert abs(gap[0] - 0.0078125) < 1e-9 and 0.0115 < eps[0] < 0.0125
    assert scope_ref.topk(exact, ok, K)[0][0, 0] == N                    # the fallback's answer is O
    _, _, mutant, _, _ = sref.certify(exact, approx, ok, N, K, ut, 1.0, sref.wmax(w), eps_scale=0.0)
    assert mutant[0]                                                     # without eps: certified, and wrong


def test_the_library_exports_the_shortlist_calls():
    from tlsan_amd import _lib as L, build
    names = ("tlsan_shortlist_build", "tlsan_shortlist_workspace_bytes", "tlsan_shortlist_topk", "tlsan_shortlist_select")
    with open(os.path.join(ROOT, "include", "tlsan.h")) as f:
        header = f.read()
    lib = L.load()
    for name in names:
        assert name in L.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    assert "tlsan_shortlist.hip" in build.SOURCES and L.ABI_VERSION == 15 and lib.tlsan_abi_version() == 15
    assert (L.SHORTLIST_NMIN, L.SHORTLIST_NMAX) == (16, 256)


def _dims(L, I=100, d=128, di=64, dc=64):
    return L.Dims(10, I, 5, d, di, dc, 8, 10)


def _params(L, **kw):
    f = dict(item_emb=FAKE, item_b=FAKE, user_emb=FAKE, usert_emb=FAKE, cate_emb=FAKE, dense=FAKE, dense_KT=FAKE, item_cate=FAKE,
             ld_item=0, ld_itemb=0, ld_user=0, ld_usert=0, scale=None, table_dtype=0, matrix_dtype=0)
    f.update(kw)
    return L.Params(*[f[n] for n, _ in L.Params._fields_])


def test_every_refusal_is_raised_on_the_host():
    from tlsan_amd import _lib as L
    lib = L.load()
    BAD, WS, UNS = -1, -2, -4

    def refused(fn, rc, code):
        assert rc == code and lib.tlsan_last_error().startswith(fn.encode()), (fn, rc, lib.tlsan_last_error())

    # ---- the workspace
    fn = "tlsan_shortlist_workspace_bytes"
    assert lib.tlsan_shortlist_workspace_bytes(5000000, 4096, 128, 64) >= 2 * 4 * 4096 * 64
    assert lib.tlsan_shortlist_workspace_bytes(15, 1, 64, 16) > 0       # one slice: still not 0, which is a refusal's
    for args in ((100, 4, 96, 64), (100, 4, 0, 64), (100, 4, 128, 15), (100, 4, 128, 257), (0, 4, 128, 64), ((1 << 30) + 1, 4, 128, 64),
                 (100, 0, 128, 64), (100, (1 << 24) + 1, 128, 64)):
        assert lib.tlsan_shortlist_workspace_bytes(*args) == 0 and lib.tlsan_last_error().startswith(fn.encode()), args
    # ---- build
    fn = "tlsan_shortlist_build"
    d, p = _dims(L), _params(L)
    good = [C.byref(d), C.byref(p), FAKE, FAKE, None]
    for i in range(4):
        a = list(good)
        a[i] = None
        refused(fn, lib.tlsan_shortlist_build(*a), BAD)
    for dims, code in ((_dims(L, d=96, di=48, dc=48), UNS), (_dims(L, d=512, di=256, dc=256), UNS), (_dims(L, di=62, dc=66), BAD),
                       (_dims(L, di=64, dc=32), BAD), (_dims(L, I=0), BAD)):
        refused(fn, lib.tlsan_shortlist_build(C.byref(dims), C.byref(p), FAKE, FAKE, None), code)
    for bad in (dict(item_emb=None), dict(cate_emb=None), dict(item_cate=None), dict(table_dtype=2)):
        q = _params(L, **bad)
        refused(fn, lib.tlsan_shortlist_build(C.byref(d), C.byref(q), FAKE, FAKE, None), BAD)
    # ---- stage 1
    fn = "tlsan_shortlist_topk"
    need = lib.tlsan_shortlist_workspace_bytes(1000, 40, 128, 64)
    good = dict(vec=FAKE, I=1000, d=128, u_t=FAKE, B=40, scale=None, item_b=FAKE, ld=1, N=64, xo=None, xi=None, mul=1, add=0,
                ids=FAKE, approx=FAKE, ws=FAKE, nws=need)

    def topk(**kw):
        a = dict(good)
        a.update(kw)
        return lib.tlsan_shortlist_topk(*([a[k] for k in good] + [None]))

    for name in ("vec", "u_t", "item_b", "ids", "approx"):
        refused(fn, topk(**{name: None}), BAD)
    for kw, code in ((dict(d=96), UNS), (dict(d=32), UNS), (dict(N=15), BAD), (dict(N=257), BAD), (dict(I=0), BAD), (dict(B=0), BAD),
                     (dict(B=(1 << 24) + 1), BAD), (dict(xo=FAKE), BAD), (dict(xi=FAKE), BAD), (dict(ld=0), BAD), (dict(mul=0), BAD),
                     (dict(add=-1), BAD), (dict(mul=1 << 22, add=5), BAD), (dict(ws=None), WS), (dict(nws=need - 1), WS), (dict(nws=0), WS)):
        refused(fn, topk(**kw), code)
    # ---- stage 2
    fn = "tlsan_shortlist_select"
    good = dict(sid=FAKE, exact=FAKE, approx=FAKE, u_t=FAKE, scale=None, wmax=FAKE, B=40, d=128, N=64, K=10, ids=FAKE, scores=FAKE,
                cert=FAKE)

    def select(**kw):
        a = dict(good)
        a.update(kw)
        return lib.tlsan_shortlist_select(*([a[k] for k in good] + [None]))

    for name in ("sid", "exact", "approx", "u_t", "wmax", "ids", "scores", "cert"):
        refused(fn, select(**{name: None}), BAD)
    for kw, code in ((dict(d=100), UNS), (dict(N=15), BAD), (dict(N=257), BAD), (dict(K=0), BAD), (dict(K=64), BAD), (dict(K=65), BAD),
                     (dict(N=16, K=16), BAD), (dict(B=0), BAD), (dict(B=(1 << 24) + 1), BAD)):
        refused(fn, select(**kw), code)


def test_value_errors_that_need_no_gpu():
    import torch
    from tlsan_amd.cluster import ClusteredIndex
    from tlsan_amd.model import CategoryIndex, ItemScope
    from tlsan_amd.shortlist import ShortlistIndex, default_shortlist, shortlist_size
    si = ShortlistIndex(torch.zeros(40, 64, dtype=torch.bfloat16), torch.ones(1))
    cat = CategoryIndex(np.arange(40) % 4, 4, "cpu")
    assert [default_shortlist(n) for n in (1, 10, 16, 17, 40, 64, 200)] == [64, 64, 64, 68, 160, 256, 256]
    assert shortlist_size(None, None, 10, 40, 64) is None and shortlist_size(cat, None, 10, 40, 64, category=[1]) is None
    assert shortlist_size(si, None, 10, 40, 64, category=None, within=None, probes=None) == 64
    assert shortlist_size(si, 16, 15, 40, 64) == 16 and shortlist_size(si, 256, 255, 40, 64) == 256 and shortlist_size(si, None, 40, 40, 64) == 160
    for args, kw in (((None, 64, 10, 40, 64), {}), ((cat, 64, 10, 40, 64), {}),            # shortlist= without a shortlist index
                     ((si, 15, 10, 40, 64), {}), ((si, 257, 10, 40, 64), {}), ((si, 64.5, 10, 40, 64), {}), ((si, True, 10, 40, 64), {}),
                     ((si, 64, 64, 40, 64), {}), ((si, 64, 100, 40, 64), {}), ((si, None, 256, 40, 64), {}),   # n < N
                     ((si, 64, 10, 41, 64), {}), ((si, 64, 10, 40, 128), {}),                 # another item count, another d
                     ((si, 64, 10, 40, 64), dict(category=[0])), ((si, 64, 10, 40, 64), dict(within=ItemScope(40, "cpu", items=[1]))),
                     ((si, 64, 10, 40, 64), dict(probes=3))):
        with pytest.raises(ValueError):
            shortlist_size(*args, **kw)
    assert si.certified is None and si.counts == (0, 0)
    si._count(torch.as_tensor([True, False, True]))
    si._count(torch.as_tensor([False]))
    assert si.counts == (4, 2) and si.certified.tolist() == [False]
    assert not isinstance(si, ClusteredIndex)


def test_sharded_models_and_the_driver_refuse_what_is_not_built():
    import torch
    from tlsan_amd import train
    from tlsan_amd.dist import ShardedModel
    from tlsan_amd.shortlist import ShortlistIndex
    si = ShortlistIndex(torch.zeros(40, 64, dtype=torch.bfloat16), torch.ones(1))
    sm = object.__new__(ShardedModel)                                     # (refused before anything of the model is looked at)
    with pytest.raises(NotImplementedError, match="per-shard"):
        sm.recommend(None, 10, index=si)
    with pytest.raises(NotImplementedError, match="per-shard"):
        sm.shortlist_index()
    a = train.parse(["--recommend_k", "10", "--shortlist_index", "1", "--shortlist", "128"])
    assert a.shortlist_index == 1 and a.shortlist == 128
    assert train.parse(["--recommend_k", "10"]).shortlist_index == 0
    for argv in (["--shortlist_index", "1"], ["--recommend_k", "10", "--shortlist", "64"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--shortlist", "15"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--shortlist", "257"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--cluster_index", "8"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--recommend_categories", "1,2"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--recommend_same_category", "1"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--sharded", "1"],
                 ["--recommend_k", "64", "--shortlist_index", "1", "--shortlist", "64"],          # the list is not shorter than the shortlist
                 ["--recommend_k", "256", "--shortlist_index", "1"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--recommend_diversity", "0.3", "--recommend_pool", "256"],
                 ["--recommend_k", "10", "--shortlist_index", "1", "--recommend_per_category", "2", "--shortlist", "32"],   # pool 40
                 ["--recommend_k", "10", "--shortlist_index", "1", "--recommend_diversity", "0.3", "--recommend_pool", "64", "--shortlist", "64"]):
        with pytest.raises(SystemExit):
            train.parse(argv)
    train.parse(["--recommend_k", "10", "--shortlist_index", "1", "--recommend_diversity", "0.3", "--recommend_pool", "64", "--shortlist", "65"])
    train.parse(["--recommend_k", "255", "--shortlist_index", "1"])
    # the certified share counts a launch's real rows, not the rows that pad it
    si._count(torch.as_tensor([True, False, True, True]))
    seen = []
    share = train.CertifiedShare(si, then=lambda db, ids, real: seen.append(real))
    share(None, None, 3)
    si._count(torch.as_tensor([False, True]))
    share(None, None, 1)
    assert share.result() == (4, 2) and seen == [3, 1] and si.counts == (6, 4)

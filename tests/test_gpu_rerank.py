"""GPU tests of the diversified lists (tlsan_rerank, Model.recommend's diversity / per_category / pool, the driver's
--recommend_diversity / --recommend_per_category / --recommend_pool) against the fp64 reference of tests/rerank_ref.py.

A near-tie may flip a greedy pick between fp32 and fp64, so with theta > 0 a returned list is not compared with the
reference's list: it is replayed step by step (rerank_ref.replay) and EVERY pick of EVERY row must have been eligible and
within tau = 8 d 2^-24 (rerank_ref.tau: derived from the fp32 rounding of the value, not measured) of the best value its
own history allowed.  With theta = 0 the selection is integer logic and the ids equal the reference's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rerank_ref as ref
from tests.helpers import batch_tuple, bits, host, make_config, random_batch, random_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 37
SPECIAL = (5, 6, 7, 8, 9)       # tail of -1 / -inf; all scores equal; two identical vectors; a zero vector; a NaN score
CASES = [(64, 16, 16, 0, 0.5), (64, 64, 20, 2, 0.3), (128, 200, 100, 3, 0.5), (256, 256, 256, 0, 0.7),
         (128, 256, 10, 1, 1.0), (64, 40, 40, 1, 0.0)]


def make_pools(d, N, seed, rows=B):
    """Made-up pools [rows, N] in tlsan_eval_topk's order: distinct ids, scores descending, vectors around 8 cluster
    centres (so the penalty binds), categories from 12 values (so the cap binds), inv = 1 / |w| rounded to fp32; and
    the five special rows."""
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((8, d))
    ids = np.stack([rng.permutation(10 * N)[:N] for _ in range(rows)]).astype(np.int32)
    s = -np.sort(-rng.standard_normal((rows, N)).astype(np.float32), 1)
    w = (centres[rng.randint(0, 8, (rows, N))] + 0.35 * rng.standard_normal((rows, N, d))).astype(np.float32)
    cate = rng.randint(0, 12, (rows, N)).astype(np.int32)
    tail = N - max(1, N // 4)
    ids[5, tail:], s[5, tail:], w[5, tail:] = -1, -np.inf, 0.0
    s[6], ids[6] = np.float32(0.75), np.sort(ids[6])                 # equal scores come in ascending id
    w[7, 3] = w[7, 1]
    w[8, 2] = 0.0
    s[9, N // 2] = np.nan
    ss = (w.astype(np.float64) ** 2).sum(2)
    inv = np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32)
    return dict(ids=ids, s=s, w=w, inv=inv, cate=cate)


def run(pool, K, m, theta, rows=None):
    """tlsan_rerank on the pools (rows: a subset, as a batch of its own) -> (ids, scores) host arrays."""
    import torch
    from tlsan_amd import _lib as L
    from tlsan_amd import model as M
    sel = slice(None) if rows is None else list(rows)
    dev = "cuda:0"
    t = {k: torch.as_tensor(np.ascontiguousarray(v[sel])).to(dev) for k, v in pool.items()}
    n, N = t["ids"].shape
    ids = torch.full((n, K), -7, dtype=torch.int32, device=dev)
    sc = torch.full((n, K), 123.0, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    M.rerank(L.load(), t["ids"], t["s"], t["w"].view(n * N, -1), t["inv"].view(-1), t["cate"].view(-1), K, theta, m, ids, sc, st)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def check_rows(pool, ids, sc, K, m, theta, d):
    """Every row and every step, teacher-forced in fp64 -> the rows that ended short."""
    short, worst = [], 0.0
    for r in range(len(ids)):
        row = [pool[k][r] for k in ("ids", "s", "w", "inv", "cate")]
        picks = ref.positions(row[0], ids[r])                        # (distinct ids of the pool, the padding last)
        regret, was, more = ref.replay(*row, theta, m, picks)
        assert was.all(), (r, picks, was)
        worst = max([worst] + regret.tolist())
        assert np.all(regret <= ref.tau(d)), (r, float(regret.max()), ref.tau(d))
        assert len(picks) == K or not more, (r, len(picks))          # a list ends early only when nothing is eligible
        assert np.array_equal(bits(sc[r, :len(picks)]), bits(row[1][picks])), r
        assert np.all(sc[r, len(picks):] == -np.inf), r
        if len(picks) < K:
            short.append(r)
    print("largest regret %.3g of tau %.3g" % (worst, ref.tau(d)))
    return short


def reference_lists(pool, K, m, theta):
    ids = np.full((len(pool["ids"]), K), -1, np.int32)
    sc = np.full((len(pool["ids"]), K), -np.inf, np.float32)
    for r in range(len(ids)):
        picks = ref.select(*[pool[k][r] for k in ("ids", "s", "w", "inv", "cate")], K, theta, m)
        ids[r, :len(picks)], sc[r, :len(picks)] = pool["ids"][r, picks], pool["s"][r, picks]
    return ids, sc


@pytest.mark.parametrize("d,N,K,m,theta", CASES)
def test_rerank_against_the_reference(d, N, K, m, theta):
    pool = make_pools(d, N, seed=1000 + N + K)
    ids, sc = run(pool, K, m, theta)
    assert ids.shape == (B, K) and ids.dtype == np.int32 and sc.dtype == np.float32
    short = check_rows(pool, ids, sc, K, m, theta, d)
    if theta == 0.0:                                                 # integer logic only: the reference's ids
        want_ids, want_sc = reference_lists(pool, K, m, theta)
        assert np.array_equal(ids, want_ids) and np.array_equal(bits(sc), bits(want_sc))
    if m > 0 and 12 * m < K:                                         # the cap ends every row short
        assert len(short) == B
    assert 5 in short or K <= N - max(1, N // 4)                     # the row with the -1 tail
    # bits: the same call again, and the special rows as a batch of their own
    ids2, sc2 = run(pool, K, m, theta)
    assert np.array_equal(ids, ids2) and np.array_equal(bits(sc), bits(sc2))
    ids5, sc5 = run(pool, K, m, theta, rows=SPECIAL)
    assert np.array_equal(ids5, ids[list(SPECIAL)]) and np.array_equal(bits(sc5), bits(sc[list(SPECIAL)]))


@pytest.mark.parametrize("d,N,K", [(64, 16, 16), (128, 200, 100), (256, 256, 256), (64, 64, 7)])
def test_rerank_identity(d, N, K):
    """theta = 0, m = 0: the pool's first K entries, ids and score bits -- on every row whose first K entries are valid
    or padding.  The row with a NaN score inside its first K is the one exception the definition itself makes (an
    invalid entry is never selected): it comes back as its valid entries in their order, the reference's list."""
    pool = make_pools(d, N, seed=2000 + N)
    ids, sc = run(pool, K, 0, 0.0)
    plain = [r for r in range(B) if r != 9 or N // 2 >= K]
    assert len(plain) >= B - 1
    assert np.array_equal(ids[plain], pool["ids"][plain, :K])
    assert np.array_equal(bits(sc[plain]), bits(pool["s"][plain, :K]))
    want_ids, want_sc = reference_lists(pool, K, 0, 0.0)
    assert np.array_equal(ids, want_ids) and np.array_equal(bits(sc), bits(want_sc))


# ---- through Model
@pytest.fixture(scope="module")
def model_case():
    from tlsan_amd.model import Model
    cfg = make_config(U=40, I=200, C=7, d=64)
    p = random_params(cfg, seed=71)
    b, cat = random_batch(cfg, B=29, Sn=3, seed=72, test=True)
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    return m, b, cat


def test_recommend_defaults_keep_the_plain_path(model_case):
    m, b, _ = model_case
    a = [host(t) for t in m.recommend(batch_tuple(b, True), 10)]
    c = [host(t) for t in m.recommend(batch_tuple(b, True), 10, diversity=0.0, per_category=0)]
    e = [host(t) for t in m.recommend(batch_tuple(b, True), 10, exclude="history", diversity=0.0, per_category=0, pool=None)]
    f = [host(t) for t in m.recommend(batch_tuple(b, True), 10, exclude="history")]
    assert np.array_equal(a[0], c[0]) and np.array_equal(bits(a[1]), bits(c[1]))
    assert np.array_equal(e[0], f[0]) and np.array_equal(bits(e[1]), bits(f[1]))
    for kw in (dict(pool=300, diversity=0.5), dict(pool=5, diversity=0.5), dict(diversity=2), dict(pool=64),
               dict(per_category=-1)):
        with pytest.raises(ValueError):
            m.recommend(batch_tuple(b, True), 10, **kw)


def test_recommend_cap_equals_the_capped_ranking_over_all_items(model_case):
    """pool = 256 holds all 200 items: the list is the brute-force capped ranking of score_candidates' scores."""
    m, b, cat = model_case
    I, n = 200, len(b["u"])
    sc_all = host(m.score_candidates(batch_tuple(b, True), np.tile(np.arange(I), (n, 1))))
    for exclude in (None, "history"):
        ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 10, exclude=exclude, per_category=2, pool=256))
        for r in range(n):
            ok = np.ones(I, bool)
            if exclude:
                ok[b["hist_i"][r, :b["sl"][r]]] = False
                ok[b["hist_i_new"][r, :b["sl_new"][r]]] = False
            want = ref.capped_ranking(sc_all[r], cat, 10, 2, ok)
            assert len(want) == 10 and ids[r].tolist() == want, (exclude, r)
            assert np.array_equal(bits(sc[r]), bits(sc_all[r, want])), (exclude, r)


@pytest.mark.parametrize("pool,N", [(None, 40), (32, 32)])
def test_recommend_diversity_passes_the_teacher_forced_check(model_case, pool, N):
    """k = 10: the default pool is min(256, max(4 k, 32)) = 40 entries, what recommend(k = 40) returns; pool = 32 picks
    from what recommend(k = 32) returns."""
    import torch
    from tlsan_amd import model as M
    m, b, cat = model_case
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 10, exclude="history", diversity=0.5, pool=pool))
    pid, psc = m.recommend(batch_tuple(b, True), N, exclude="history")
    vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, pid.reshape(-1).contiguous(), 1, 0, m._stream())
    torch.cuda.synchronize()
    n = len(b["u"])
    pid_h = host(pid)
    pl = dict(ids=pid_h, s=host(psc), w=host(vec).reshape(n, N, -1), inv=host(inv).reshape(n, N),
              cate=np.asarray(cat)[np.maximum(pid_h, 0)])
    assert check_rows(pl, ids, sc, 10, 0, 0.5, 64) == []
    plain = host(m.recommend(batch_tuple(b, True), 10, exclude="history")[0])
    assert np.array_equal(ids[:, 0], plain[:, 0]) and not np.array_equal(ids, plain)     # the penalty moved something


def test_driver_writes_capped_recommendations(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "3",
                        "--eval_freq", "1000", "--quiet", "--recommend_k", "5", "--recommend_per_category", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(os.path.join(out, "recommend_top5.npz"))
    assert float(z["diversity"]) == 0.0 and int(z["per_category"]) == 1 and int(z["pool"]) == 0
    cat = np.load(ds)["item_cate_list"]
    ids = z["ids"]
    assert ids.shape[1] == 5 and z["scores"].shape == ids.shape and (ids >= 0).any()
    for row in ids:
        c = cat[row[row >= 0]]
        assert len(set(c.tolist())) == len(c), row

"""GPU tests of the similar-items lists (tlsan_item_vectors / tlsan_similar_topk, Model.similar_items,
ShardedModel.similar_items, the driver's --similar_k) against the numpy reference of tests/similar_ref.py: both metrics
within the fp32 bound, the exact order on integer tables, eligibility, independence of the launch, symmetry in bits, the
lazy-L2 state, bf16 tables, the gathering form past the dense cap, the sharded form bit for bit, and the driver."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import similar_ref as ref
from tests.helpers import bits, make_config, model, random_batch, random_params, sharded
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = ("cosine", "dot")


def _params(cfg, seed, **tables):
    p = {k: np.asarray(v, np.float32) for k, v in random_params(cfg, seed=seed).items()}
    for k, v in tables.items():
        assert v.shape == p[k].shape, k
        p[k] = np.asarray(v, np.float32)
    return p


def _model(cfg, cat, p, **kw):
    m = model(cfg, cat, **kw)
    m.set_params(p)          # (float32 as _params made them, handed over unconverted: helpers.model would convert)
    return m


def _cat(cfg, seed=5):
    return np.random.RandomState(seed).randint(0, cfg["cate_count"], cfg["item_count"]).astype(np.int32)


def _stored(m, cat):
    """the item matrix as the tables hold it now (bf16 widened exactly), in fp64"""
    return ref.item_matrix(m.item_emb.float().cpu().numpy(), m.cate_emb.float().cpu().numpy(), cat)


def _host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _check(m, w, qids, k, metric, exclude=None, P=1.0, got=None):
    ids, sc = _host(m.similar_items(qids, k, metric=metric, exclude=exclude)) if got is None else got
    assert ids.shape == (len(qids), k) and ids.dtype == np.int32
    ref.check_lists(ids, sc, ref.scores(w, qids, metric, P), ref.eligible(w.shape[0], qids, exclude),
                    ref.tolerance(w, qids, metric, P))
    return ids, sc


# ---- 1. against numpy, both metrics
@pytest.mark.parametrize("I", [1, 15, 257, 1000])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_similar_matches_numpy(d, I):
    cfg = make_config(U=8, I=I, C=5, d=d, H=8)              # many items per category
    cat = _cat(cfg)
    m = _model(cfg, cat, _params(cfg, seed=11 + d + I))
    w = _stored(m, cat)
    qall = np.random.RandomState(I).randint(0, I, 33)
    for Q in (1, 17, 33):
        for k in (5, 16, 17, 64, 65, 256):                  # each dispatch class and its edges; k > eligible for small I
            for metric in METRICS:
                _check(m, w, qall[:Q], k, metric)


# ---- 2. exact order
def _int_tables(cfg, seed):
    rng = np.random.RandomState(seed)
    di, dc = cfg["itemid_embedding_size"], cfg["cateid_embedding_size"]
    return dict(item_emb=rng.randint(-3, 4, (cfg["item_count"], di)).astype(np.float32),
                cate_emb=rng.randint(-3, 4, (cfg["cate_count"], dc)).astype(np.float32))


def _exact(m, w, qids, k, metric="dot"):
    s = ref.scores(w, qids, metric)
    want_ids, want_sc = ref.topk(s, ref.eligible(w.shape[0], qids), k)
    ids, sc = _host(m.similar_items(qids, k, metric=metric))
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(sc, want_sc.astype(np.float32))


@pytest.mark.parametrize("d", [64, 256])
def test_exact_order_on_integer_tables(d):
    cfg = make_config(U=8, I=700, C=4, d=d, H=8)
    cat = _cat(cfg)
    m = _model(cfg, cat, _params(cfg, seed=21, **_int_tables(cfg, 22)))
    w = _stored(m, cat)
    assert np.array_equal(w, np.rint(w))
    qids = np.arange(0, 700, 37)
    for k in (5, 64, 256):                                   # integer scores in a narrow range: ties everywhere
        _exact(m, w, qids, k)


def test_duplicate_rows_under_cosine():
    cfg = make_config(U=8, I=90, C=3, d=64, H=8)
    rng = np.random.RandomState(31)
    base = rng.uniform(-1, 1, (6, 32)).astype(np.float32)
    cat = (np.arange(90) % 6 % 3).astype(np.int32)           # copies of a row share its category
    m = _model(cfg, cat, _params(cfg, seed=32, item_emb=base[np.arange(90) % 6]))
    w = _stored(m, cat)
    qids = np.array([0, 7, 89, 7])
    ids, sc = _check(m, w, qids, 20, "cosine")
    for r, q in enumerate(qids):
        copies = [n for n in range(90) if n % 6 == q % 6 and n != q]
        assert ids[r, :14].tolist() == copies                # 14 bit-identical rows: ascending id, never the query
        assert len(set(bits(sc[r, :14]).tolist())) == 1
    assert np.array_equal(ids[1], ids[3]) and np.array_equal(bits(sc[1]), bits(sc[3]))


def test_scores_rising_with_the_id_overflow_the_buffers():
    I = 3001
    cfg = make_config(U=8, I=I, C=3, d=64, H=8)
    item = np.zeros((I, 32), np.float32)
    item[:, 0] = np.arange(I)                                # s(q, n) = q n: every later item beats the threshold
    item[0, 0] = 1
    item[:, 1] = np.arange(I) % 3 - 1
    cat = _cat(cfg)
    m = _model(cfg, cat, _params(cfg, seed=41, item_emb=item, cate_emb=np.zeros((3, 32), np.float32)))
    w = _stored(m, cat)
    for k in (16, 64, 200):
        _exact(m, w, np.array([0, 1, 5, 3000]), k)


# ---- 3. eligibility
def _c_call(m, qids, k, metric, excl=(None, None)):
    """tlsan_item_vectors + tlsan_similar_topk as Model.similar_items makes them, without its checks of the ids"""
    import torch
    from tlsan_amd import model as M
    q = torch.as_tensor(np.asarray(qids, np.int32)).to(m.device)
    vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, q, 1, 0, m._stream())
    out = M.similar_topk(m.lib, m.dims, m.cparams, vec, inv, q, k, M.SIMILAR_METRICS[metric], excl, 1, 0,
                         m._topk_workspace, m._stream())
    return vec.cpu().numpy(), inv.cpu().numpy(), _host(out)


def test_eligibility():
    import torch
    I = 300
    cfg = make_config(U=8, I=I, C=6, d=128, H=8)
    cat = _cat(cfg)
    cat[17] = 5
    cat = np.where((cat == 5) & (np.arange(I) != 17), 0, cat).astype(np.int32)     # item 17 alone in category 5
    p = _params(cfg, seed=51)
    p["item_emb"][17] = 0
    p["cate_emb"][5] = 0                                     # a zero row
    m = _model(cfg, cat, p)
    w = _stored(m, cat)
    assert not w[17].any()
    qids = np.array([3, 17, 3, 299, 40])
    excl = [[5, 5, 9, 100000, -7, 250], [], [5, 9, 250], list(range(0, 299)), [40, 41]]
    for metric in METRICS:
        for k in (5, 64, 256):
            ids, sc = _check(m, w, qids, k, metric, exclude=excl)
            assert np.array_equal(ids[0], ids[2]) and np.array_equal(bits(sc[0]), bits(sc[2]))   # the same query twice
            assert ids[3].tolist() == [-1] * k               # everything but the query excluded
        with pytest.raises(ValueError):
            m.similar_items([3, I], 5, metric=metric)
        with pytest.raises(ValueError):
            m.similar_items([-1], 5, metric=metric)
    with pytest.raises(ValueError):
        m.similar_items([3], 5, metric="l2")
    with pytest.raises(ValueError):
        m.similar_items([3, 4], 5, exclude=[[1]])
    # the zero row: inv = 0, every score +0.0, ids ascending
    ids, sc = _host(m.similar_items([17], 8, metric="cosine"))
    assert ids[0].tolist() == list(range(8)) and np.array_equal(bits(sc), np.zeros((1, 8), np.int32))
    # a padding query and an id past the table, through the C call; foreign and repeated ids in the CSR itself
    off = torch.tensor([0, 4, 4, 4, 7], dtype=torch.int32, device=m.device)
    xid = torch.tensor([5, 5, 9, 2 ** 31 - 1, 8, 8, 1 << 20], dtype=torch.int32, device=m.device)
    vec, inv, (ids, sc) = _c_call(m, [3, -1, 17, I + 5], 7, "cosine", (off, xid))
    assert inv[2] == 0 and inv[1] == 0 and inv[3] == 0 and not vec[1].any() and not vec[3].any()
    assert np.array_equal(vec[0], w[3].astype(np.float32))
    assert abs(inv[0] - 1 / np.sqrt((w[3] ** 2).sum())) <= (128 / 2 + 2) * ref.U * inv[0]
    for r in (1, 3):
        assert ids[r].tolist() == [-1] * 7 and np.all(sc[r] == -np.inf)
    _check(m, w, np.array([3]), 7, "cosine", exclude=[[5, 9]], got=(ids[:1], sc[:1]))


# ---- 4. independence and symmetry
def test_independence_and_symmetry():
    I = 257
    cfg = make_config(U=8, I=I, C=5, d=128, H=8)
    cat = _cat(cfg)
    m = _model(cfg, cat, _params(cfg, seed=61))
    qids = np.random.RandomState(62).randint(0, I, 33)
    for metric in METRICS:
        many = _host(m.similar_items(qids, 20, metric=metric))
        again = _host(m.similar_items(qids, 20, metric=metric))
        assert np.array_equal(many[0], again[0]) and np.array_equal(bits(many[1]), bits(again[1]))
        for r in (0, 16, 32):
            one = _host(m.similar_items(qids[r:r + 1], 20, metric=metric))
            assert np.array_equal(one[0][0], many[0][r]) and np.array_equal(bits(one[1][0]), bits(many[1][r]))
        ids, sc = _host(m.similar_items(np.arange(I), 256, metric=metric))      # every pair, both ways round
        S = np.zeros((I, I), np.int32)
        S[np.arange(I)[:, None], ids] = bits(sc)
        assert np.all(np.sort(ids, 1) == np.delete(np.tile(np.arange(I), (I, 1)), np.arange(I) * (I + 1)).reshape(I, I - 1))
        assert np.array_equal(S, S.T)


@pytest.mark.parametrize("k", [16, 17, 256])
def test_topk_on_the_queries_vectors_equals_dot(k):
    """k_eval_topk and k_similar_topk are two texts of one scan (k_eval_topk's own, and topk_scan with SimScore) that
    must stay the same tiles and the same selection; this is the guard that they do.  With P = 1 and no bias the
    recommendation score of u_t = the queries' stored vectors IS the dot product, so excluding each row's own id gives
    the dot lists, ids and scores.  I = 300: the last 64-item group is partial; Q = 20: so is the second row tile."""
    import torch
    from tlsan_amd import model as M
    I = 300
    cfg = make_config(U=8, I=I, C=5, d=64, H=8)
    cat = _cat(cfg)
    p = _params(cfg, seed=111)
    p["item_b"] = np.zeros_like(p["item_b"])
    m = _model(cfg, cat, p)
    assert m.table_scale() == 1.0
    qids = np.random.RandomState(112).randint(0, I, 20)
    qids[7] = I + 5                                          # no row of the table: nothing to compare
    vec, _, (sid, ssc) = _c_call(m, qids, k, "dot")
    own = (torch.arange(21, dtype=torch.int32, device=m.device), torch.as_tensor(qids.astype(np.int32)).to(m.device))
    tid, tsc = _host(M.eval_topk(m.lib, m.dims, m.cparams, torch.as_tensor(vec).to(m.device), 20, k, own, 1, 0,
                                 m._topk_workspace, m._stream()))
    rows = np.arange(20) != 7
    assert sid[7].tolist() == [-1] * k and (sid[rows] >= 0).all()
    assert np.array_equal(tid[rows], sid[rows])
    assert np.array_equal(tsc[rows], ssc[rows])              # (==: a zero of either sign is a zero)


# ---- 5. the lazy-L2 state
def test_lazy_l2_state_is_read_not_changed():
    cfg = make_config(U=40, I=500, C=7, d=128, H=8)
    tb, cat = random_batch(cfg, B=64, Sn=3, seed=72)
    m = _model(cfg, cat, _params(cfg, seed=71), l2_mode="lazy")
    for _ in range(3):
        m.train(None, (tb["u"], tb["i"], tb["y"], tb["hist_i"], tb["hist_i_new"], tb["hist_t"], tb["sl"], tb["sl_new"],
                       tb["u_cate"]), 1.0)
    qids = np.arange(0, 500, 23)
    m.similar_items(qids, 5)                                 # (what the last step owed lands with the first call)
    P = m.table_scale()
    assert P != 1.0
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.cate_emb, m.item_b, m.dense)]
    before = snap()
    w = _stored(m, cat)
    for metric in METRICS:
        _check(m, w, qids, 30, metric, P=P)
    after = snap()
    assert m.table_scale() == P
    import torch
    assert all(torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)) for a, b in zip(before, after))


# ---- 6. bf16 tables
def test_bf16_tables():
    cfg = make_config(U=8, I=257, C=5, d=128, H=8)
    cat = _cat(cfg)
    m = _model(cfg, cat, _params(cfg, seed=81), table_dtype="bf16")
    w = _stored(m, cat)
    assert np.array_equal(bits(w.astype(np.float32)) & 0xFFFF, np.zeros(w.shape, np.int32))
    for Q in (1, 33):
        for k in (16, 65):
            for metric in METRICS:
                _check(m, w, np.arange(Q) * 7, k, metric)


# ---- 7. the gathering form, just past the dense cap
def test_gathering_form_past_the_dense_cap():
    I = (1 << 20) + 3                                        # I * 64 * 4 B > 256 MB
    cfg = make_config(U=8, I=I, C=50, d=64, H=8)
    rng = np.random.RandomState(91)
    cat = rng.randint(0, 50, I).astype(np.int32)
    p = _params(make_config(U=8, I=4, C=50, d=64, H=8), seed=92)
    p["item_emb"] = rng.uniform(-0.8, 0.8, (I, 32)).astype(np.float32)
    p["item_b"] = np.zeros((I,) + p["item_b"].shape[1:], np.float32)
    m = _model(cfg, cat, p)
    w = _stored(m, cat)
    for metric in METRICS:
        _check(m, w, np.array([0, I - 1, 524288]), 16, metric)


def test_gathering_form_at_d256():
    """d = 256 past the dense cap with K <= 16 and K <= 64: the two instantiations under the most register pressure"""
    I = (1 << 18) + 3                                        # I * 256 * 4 B > 256 MB
    cfg = make_config(U=8, I=I, C=50, d=256, H=8)
    rng = np.random.RandomState(93)
    cat = rng.randint(0, 50, I).astype(np.int32)
    p = _params(make_config(U=8, I=4, C=50, d=256, H=8), seed=94)
    p["item_emb"] = rng.uniform(-0.8, 0.8, (I, 128)).astype(np.float32)
    p["item_b"] = np.zeros((I,) + p["item_b"].shape[1:], np.float32)
    m = _model(cfg, cat, p)
    w = _stored(m, cat)
    for metric in METRICS:
        for k in (16, 64):
            _check(m, w, np.array([0, I - 1, 131072]), k, metric)


# ---- 8. sharded
def _sharded_case(rank, world):
    I = 257                                                  # not a multiple of the world size
    cfg = make_config(U=20, I=I, C=5, d=128, H=8)
    cat = _cat(cfg)
    p = _params(cfg, seed=101)
    p["item_emb"][::3, ::5] = -0.0
    p["cate_emb"][1, :7] = -0.0
    sm = sharded(cfg, cat, p, l2_mode="dense")
    m = _model(cfg, cat, {k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    assert np.signbit(m.item_emb.cpu().numpy()[0, 0]) and np.signbit(m.cate_emb.cpu().numpy()[1, 0])
    qids = np.random.RandomState(102).randint(0, I, 33)
    excl = [list(np.random.RandomState(r).randint(-2, I + 9, r % 5 * 3)) for r in range(33)]
    w = _stored(m, cat)
    for metric in METRICS:
        for k, ex in ((5, None), (64, excl), (256, excl)):
            want = _host(m.similar_items(qids, k, metric=metric, exclude=ex))
            got = _host(sm.similar_items(qids, k, metric=metric, exclude=ex))
            assert np.array_equal(got[0], want[0]), (metric, k)
            assert np.array_equal(bits(got[1]), bits(want[1])), (metric, k)
            _check(m, w, qids, k, metric, exclude=ex, got=got)


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_similar_items_equal_the_model_bit_for_bit(world):
    run_ranks(_sharded_case, world)


# ---- 9. the driver
def test_driver_writes_similar_items(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "5",
                        "--eval_freq", "1000", "--similar_k", "5"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    path = os.path.join(out, "similar-5.npz")
    assert "Similar items: %s" % path in r.stdout
    _check_file(path, ds)


def _check_file(path, ds):
    z = np.load(path)
    I = int(np.load(ds)["counts"][1])
    item, ids, sc = z["item"], z["ids"], z["scores"]
    assert np.array_equal(item, np.arange(I)) and ids.shape == (I, 5) and sc.shape == (I, 5) and sc.dtype == np.float32
    assert ids.min() >= 0 and ids.max() < I
    assert np.all(ids != item[:, None])
    assert all(len(set(row.tolist())) == 5 for row in ids)
    a, b = sc[:, :-1], sc[:, 1:]
    assert np.all((a > b) | ((a == b) & (ids[:, :-1] < ids[:, 1:])))
    assert np.all(np.abs(sc) <= 1 + 1e-5)                    # cosine


def _sharded_driver_worker(rank, world, out):
    from tlsan_amd import train as T
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    T.train_sharded(T.parse(["--dataset", ds, "--max_steps", "5", "--eval_freq", "1000", "--quiet", "--train_batch_size", "33",
                             "--model_dir", os.path.join(out, "r%d" % rank), "--device_input", "0", "--l2_mode", "lazy",
                             "--static_rows", "1", "--similar_k", "5", "--sharded", "1"]))
    path = os.path.join(out, "r%d" % rank, "similar-5.npz")
    assert os.path.exists(path) == (rank == 0)           # rank 0 writes
    if rank == 0:
        _check_file(path, ds)


def test_sharded_driver_writes_similar_items(tmp_path):
    run_ranks(_sharded_driver_worker, 2, str(tmp_path))

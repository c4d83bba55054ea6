"""Audience lists on the GPU: Model.audience against the reference order applied to Model.score_candidates' own [N, Q]
scores -- ids and score BITS, no tolerance: a row appears in an item's audience with exactly the score the item has in
that row's list -- the raw tlsan_dense_topk on hand-made integer matrices (ties, id_add, zeros, NaN, inf, exclusion
lists, more than one slice, more than one round), the SeenItems exclusion, determinism, the state left as it was, the
refusals and the driver."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import audience_ref as ref
from tests.helpers import batch_tuple, bits, host, make_config, model, random_batch, random_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 16, 17, 257, 600)    # one row, a full tile, a partial one, two slices (a merge), three
QS = (1, 17, 40)
KS = (1, 10, 64, 100)           # the three forms of TOPK_DISPATCH (<= 16, <= 64, above); 64 and 100 exceed the small row counts
I = 300


@functools.lru_cache(maxsize=None)
def _case(d, heads, state):
    """(model, its 600-row test batch as a dict): `dense` -- dense L2, P = 1; `lazy` -- lazy L2 after three training
    steps, P != 1; `bf16` -- the lazy one with bf16 tables."""
    cfg = make_config(U=50, I=I, C=9, d=d, H=heads)
    p = random_params(cfg, seed=d + heads)
    b, cat = random_batch(cfg, B=max(ROWS), Sn=3, seed=d + 1, test=True)
    if state == "dense":
        return model(cfg, cat, p), b
    m = model(cfg, cat, p, l2_mode="lazy", table_dtype="bf16" if state == "bf16" else "f32")
    tb, _ = random_batch(cfg, B=128, Sn=3, seed=d + 2)
    for _ in range(3):
        m.train(None, batch_tuple(tb), 1.0)
    assert m.table_scale() != 1.0
    return m, b


def _rows(b, n):
    return batch_tuple({k: v[:n] for k, v in b.items()}, True)


def _items(Q, seed):
    items = np.random.RandomState(seed).randint(0, I, Q)
    if Q > 1:
        items[-1] = items[0]                                          # a repeated item
    return items


def _same(got, want, what):
    rows, sc = host(got[0]), host(got[1])
    assert rows.dtype == np.int32 and sc.dtype == np.float32 and rows.shape == want[0].shape, what
    assert np.array_equal(rows, want[0]), what
    assert np.array_equal(bits(sc), bits(want[1])), what


@pytest.mark.parametrize("d,heads,state", [(64, 4, "dense"), (128, 8, "dense"), (256, 8, "dense"),
                                           (64, 4, "lazy"), (128, 8, "lazy"), (256, 8, "lazy"), (128, 8, "bf16")])
def test_audience_scores_are_the_scorers_bits(d, heads, state):
    m, b = _case(d, heads, state)
    for n in ROWS:
        batch = _rows(b, n)
        users = m.user_vectors(batch)
        assert len(users) == n and users.row0 == 0 and users.n_total == n
        assert np.array_equal(host(users.user), b["u"][:n].astype(np.int32))
        for Q in QS:
            items = _items(Q, n + Q)
            s = host(m.score_candidates(batch, np.tile(items, (n, 1))))           # the parent's scorer: [n, Q] fp32
            assert s.shape == (n, Q) and np.isfinite(s).all()
            for k in KS:
                got = m.audience(items, k, users)
                _same(got, ref.expected(s.T, k), (n, Q, k))
                if k > n:
                    assert (host(got[0])[:, n:] == -1).all() and (host(got[1])[:, n:] == -np.inf).all()
                assert np.array_equal(host(users.users_of(got[0])),
                                      np.where(host(got[0]) >= 0, b["u"][np.maximum(host(got[0]), 0)], -1))


def test_user_vectors_of_several_batches_and_kept_rows():
    import torch
    m, b = _case(128, 8, "dense")
    parts = [batch_tuple({k: v[lo:hi] for k, v in b.items()}, True) for lo, hi in ((0, 33), (33, 34), (34, 100))]
    each = [m.forward(part, is_test=True, want_u_t=True)[2] for part in parts]       # what forward gives for each batch ...
    joined = m.user_vectors(parts)                                                   # ... concatenated in the order given
    assert np.array_equal(bits(host(joined.vec)), bits(host(torch.cat(each))))
    assert np.array_equal(host(joined.user), b["u"][:100].astype(np.int32)) and (joined.row0, joined.n_total) == (0, 100)
    kept = m.user_vectors([m.device_batch(parts[0], is_test=True), parts[2]], real=[10, 0])   # (a DeviceBatch; padded launches)
    assert len(kept) == 10 and np.array_equal(bits(host(kept.vec)), bits(host(each[0])[:10]))
    items = _items(5, 3)
    s = np.concatenate([host(m.score_candidates(part, np.tile(items, (len(part[0]), 1)))) for part in parts])
    _same(m.audience(items, 10, joined), ref.expected(s.T, 10), "joined")


def _raw(m, q, x, scale, bias, excl, id_add, k):
    """tlsan_dense_topk itself, all Q queries in one call (model.dense_topk goes 4096 at a time)."""
    import torch
    from tlsan_amd import _lib as L
    dev = m.device
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dt)).to(dev)
    tq, tx, ts, tb = up(q, np.float32), up(x, np.float32), up(scale, np.float32), up(bias, np.float32)
    off = xid = None
    if excl is not None:
        off = up(np.cumsum([0] + [len(e) for e in excl]), np.int32)
        xid = up(np.concatenate([np.sort(np.asarray(e, np.int64)) for e in excl] + [np.zeros(1, np.int64)]), np.int32)
    Q, N = q.shape[0], x.shape[0]
    ids = torch.empty(Q, k, dtype=torch.int32, device=dev)
    sc = torch.empty(Q, k, dtype=torch.float32, device=dev)
    ws = torch.empty(m.lib.tlsan_dense_topk_workspace_bytes(Q, N, k), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(m.lib.tlsan_dense_topk(tq.data_ptr(), Q, q.shape[1], tx.data_ptr(), N, ptr(ts), ptr(tb), ptr(off), ptr(xid), id_add,
                                   k, ids.data_ptr(), sc.data_ptr(), ws.data_ptr(), ws.numel(), m._stream()), "tlsan_dense_topk")
    return host(ids), host(sc)


def _want(q, x, scale, bias):
    """Small-integer entries: fp64 numpy gives the fp32 accumulator, the scaled value and the sum exactly."""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = q.astype(np.float64) @ x.astype(np.float64).T
        s = acc * (1.0 if scale is None else scale.astype(np.float64)[:, None])
        s = s + (0.0 if bias is None else bias.astype(np.float64)[:, None])
    return s.astype(np.float32)


def _check_raw(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    nan = np.isnan(want[1])
    assert np.array_equal(np.isnan(got[1]), nan), what
    assert np.array_equal(bits(got[1])[~nan], bits(want[1])[~nan]), what


@pytest.mark.parametrize("d", [64, 128, 256])
def test_raw_call_on_hand_made_matrices(d):
    m, _ = _case(128, 8, "dense")
    rng = np.random.RandomState(d)
    N, Q, id_add = 300, 21, 1000                                      # two slices and a merge; a partial query tile
    x = rng.randint(-2, 3, (N, d)).astype(np.float32)
    q = rng.randint(-2, 3, (Q, d)).astype(np.float32)
    q[:, 0] = 1.0                                                     # (column 0 carries the inf and the NaN below)
    x[40] = x[7]; x[299] = x[7]; x[8] = x[7]                          # duplicate rows: a tie goes to the lower row
    x[100] = 0.0                                                      # a zero row
    x[200, 0] = np.nan                                                # a NaN row: last
    x[250, 0] = np.inf                                                # a +inf score for every query
    scale = rng.choice([0.5, 1.0, 2.0, 4.0], Q).astype(np.float32)
    bias = rng.randint(-3, 4, Q).astype(np.float32)
    scale[3], bias[3] = 1.0, -0.0                                     # zero row, bias -0.0: the score is returned as +0.0
    excl = [[] for _ in range(Q)]                                     # empty lists
    excl[1] = list(range(id_add, id_add + N))                         # every row: all -1 / -inf
    excl[2] = [5, 999, id_add + N, 2 ** 31 - 1]                       # ids outside the range: ignored
    excl[4] = [7, 8, id_add + 7, id_add + 250, id_add + 100]          # (7 and 8 are outside: rows 1007, 1250 and 1100 go)
    s = _want(q, x, scale, bias)
    for k in (1, 10, 100, 256):
        got = _raw(m, q, x, scale, bias, excl, id_add, k)
        _check_raw(got, ref.expected(s, k, excl, id_add), ("excl", k))
        assert (got[0][1] == -1).all() and (got[1][1] == -np.inf).all()
        assert (got[0][[0, 2, 3]][:, 0] == id_add + 250).all() and (got[1][[0, 2, 3]][:, 0] == np.inf).all()
        assert id_add + 250 not in got[0][4] and id_add + 7 not in got[0][4]
        _check_raw(_raw(m, q, x, scale, bias, None, id_add, k), ref.expected(s, k, None, id_add), ("plain", k))
    got = _raw(m, q, x, None, None, None, 0, 256)                     # scale and bias NULL: 1 and 0
    _check_raw(got, ref.expected(_want(q, x, None, None), 256), "null")
    tied = 0
    for qi in range(Q):                                               # the four equal rows, wherever a list holds them all
        at = [list(got[0][qi]).index(r) for r in (7, 8, 40, 299) if r in got[0][qi]]
        if len(at) == 4:
            tied += 1
            assert at == sorted(at) and len(set(bits(got[1][qi][at]).tolist())) == 1, qi
    assert tied > 0
    got = _raw(m, q, x, scale, bias, None, 0, 256)
    z = list(got[0][3]).index(100)
    assert got[1][3][z] == 0.0 and not np.signbit(got[1][3][z])
    full = _raw(m, q[:2], x[:250], None, None, None, 0, 256)          # N < K, the NaN row last, then the padding
    assert full[0][0][249] == 200 and np.isnan(full[1][0][249]) and (full[0][:, 250:] == -1).all() and (full[1][:, 250:] == -np.inf).all()


def test_raw_call_with_more_than_one_round():
    # 4101 queries are 257 tiles: 8 slices fill the chip; 2100 rows are 9 groups of 256, so a slice takes a second round
    m, _ = _case(128, 8, "dense")
    rng = np.random.RandomState(11)
    base, N, Q = 41, 2100, 4101
    x = rng.randint(-2, 3, (N, 64)).astype(np.float32)
    qb = rng.randint(-2, 3, (base, 64)).astype(np.float32)
    sb, bb = rng.choice([0.5, 1.0, 2.0], base).astype(np.float32), rng.randint(-3, 4, base).astype(np.float32)
    pick = np.arange(Q) % base
    for k in (10, 100):
        want = ref.expected(_want(qb, x, sb, bb), k, None, 5)
        got = _raw(m, qb[pick], x, sb[pick], bb[pick], None, 5, k)
        assert np.array_equal(got[0], want[0][pick]) and np.array_equal(bits(got[1]), bits(want[1][pick])), k


def test_seen_items_exclusion():
    from tlsan_amd.model import SeenItems
    m, b = _case(128, 8, "lazy")
    rng = np.random.RandomState(21)
    U = m.config["user_count"]
    seen = [np.sort(rng.choice(I, rng.randint(0, 60), replace=False)) for _ in range(U)]
    seen[3] = np.zeros(0, np.int64)
    off, ids = np.cumsum([0] + [len(x) for x in seen]), np.concatenate(seen)
    holder = SeenItems(off, ids, m.device)
    n = 600
    batch = _rows(b, n)
    users = m.user_vectors(batch)                                     # 600 rows of 50 users: users with several rows
    items = np.concatenate([seen[0][:6], seen[7][:6], _items(5, 9)])
    s = host(m.score_candidates(batch, np.tile(items, (n, 1))))
    gone = ref.seen_rows(off, ids, b["u"][:n], items)
    assert sum(len(g) for g in gone) > 50
    for k in (10, 100):
        got = m.audience(items, k, users, exclude=holder)
        _same(got, ref.expected(s.T, k, gone), k)
        who = host(users.users_of(got[0]))
        for qi, it in enumerate(items):
            assert all(it not in seen[u] for u in who[qi] if u >= 0), (qi, it)
    listed = [rng.randint(-3, n + 5, qi % 4 * 40) for qi in range(len(items))]          # explicit lists of row numbers
    _same(m.audience(items, 64, users, exclude=listed), ref.expected(s.T, 64, listed), "listed")


def test_deterministic_and_nothing_changes():
    import torch
    m, b = _case(256, 8, "lazy")
    snap = lambda: [t.clone() for t in (m.state, m.item_emb, m.item_b, m.user_emb, m.usert_emb, m.cate_emb, m.dense, m.dense_KT)]
    scale, before = m.table_scale(), snap()
    items = _items(17, 5)
    users = m.user_vectors(_rows(b, 257))
    one = [host(t) for t in m.audience(items, 64, users)]
    users2 = m.user_vectors(_rows(b, 257))
    two = [host(t) for t in m.audience(items, 64, users2)]
    assert np.array_equal(bits(host(users.vec)), bits(host(users2.vec)))
    assert np.array_equal(one[0], two[0]) and np.array_equal(bits(one[1]), bits(two[1]))
    after = snap()
    assert m.table_scale() == scale
    assert all(torch.equal(a.reshape(-1).view(torch.uint8), c.reshape(-1).view(torch.uint8)) for a, c in zip(before, after))


def test_refusals():
    from tlsan_amd.model import UserVectors
    cfg = make_config(U=50, I=I, C=9, d=64, H=4)
    p = random_params(cfg, seed=1)
    b, cat = random_batch(cfg, B=40, Sn=3, seed=2, test=True)
    tb, _ = random_batch(cfg, B=32, Sn=3, seed=3)
    m, other = model(cfg, cat, p), model(cfg, cat, p)
    users = m.user_vectors(batch_tuple(b, True))
    m.audience([1, 2], 5, users)
    calls = []
    real = m.lib.tlsan_dense_topk
    m.lib.tlsan_dense_topk = lambda *a: calls.append(a) or real(*a)          # (counts the launches the refusals must not reach)
    try:
        for items, k, uv, ex in (([1], 0, users, None), ([1], 257, users, None), ([I], 5, users, None), ([-1], 5, users, None),
                                 ([], 5, users, None), ([[1, 2]], 5, users, None),
                                 ([1], 5, host(users.vec), None), ([1], 5, other.user_vectors(batch_tuple(b, True)), None),
                                 ([1], 5, UserVectors(users.vec[:, :32], users.user, m, m._step), None),
                                 ([1], 5, UserVectors(users.vec.cpu(), users.user.cpu(), m, m._step), None),
                                 ([1], 5, users, "history"), ([1, 2], 5, users, [[0]])):
            with pytest.raises(ValueError):
                m.audience(items, k, uv, exclude=ex)
        with pytest.raises(ValueError):
            m.user_vectors([])
        m.train(None, batch_tuple(tb), 1.0)                               # one more training step: the vectors are stale
        with pytest.raises(ValueError, match="rebuild"):
            m.audience([1, 2], 5, users)
        assert not calls
        m.audience([1, 2], 5, m.user_vectors(batch_tuple(b, True)))      # rebuilt: accepted again
        assert len(calls) == 1
    finally:
        m.lib.tlsan_dense_topk = real


def test_driver_writes_audiences(tmp_path):
    from tlsan_amd.input import seen_items_csr
    from tlsan_amd.train import load_dataset
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    train_set, test_set, (U, n_items, _), _ = load_dataset(ds)
    off, ids = seen_items_csr(train_set, U)
    busy = np.bincount(ids, minlength=n_items).argsort()[::-1][:3]        # items many users have seen: the exclusion bites
    items = [int(busy[0]), int(busy[1]), 0, int(busy[2]), int(busy[0])]
    r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", out, "--max_steps", "5",
                        "--eval_freq", "1000", "--audience_k", "5", "--audience_items", ",".join(map(str, items)),
                        "--audience_exclude", "seen"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    path = os.path.join(out, "audience-5.npz")
    assert "Audience: %s" % path in r.stdout
    z = np.load(path)
    assert sorted(z.files) == ["item", "rows", "scores", "users"]
    item, users, rows, sc = z["item"], z["users"], z["rows"], z["scores"]
    assert np.array_equal(item, items) and users.shape == rows.shape == sc.shape == (5, 5)
    assert rows.dtype == np.int32 and users.dtype == np.int32 and sc.dtype == np.float32
    assert rows.min() >= 0 and rows.max() < len(test_set) and all(len(set(x.tolist())) == 5 for x in rows)
    a, c = sc[:, :-1], sc[:, 1:]
    assert np.all((a > c) | ((a == c) & (rows[:, :-1] < rows[:, 1:])))
    assert np.array_equal(rows[0], rows[4]) and np.array_equal(bits(sc[0]), bits(sc[4]))     # the repeated item
    for qi, it in enumerate(items):
        for u in users[qi]:
            assert 0 <= u < U and it not in ids[off[u]:off[u + 1]], (qi, it, u)

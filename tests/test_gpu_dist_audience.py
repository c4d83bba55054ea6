"""ShardedModel.user_vectors / audience with one rank and with two (two processes share cuda:0 and talk over gloo): every
rank's lists against the reference order over the ranks' gathered ShardedModel.score_candidates scores -- ids and score
bits -- with unequal row counts, a rank without rows, exclusion lists and a SeenItems holder; users_of returns the
gathered user ids.  And the sharded driver: rank 0 alone writes the file."""
import os

import numpy as np
import pytest

from tests import audience_ref as ref
from tests.helpers import batch_tuple, bits, host, make_config, random_batch, random_params, sharded
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I = 257                         # items not a multiple of the world size
LAUNCH = 40                     # rows every rank hands to a forward (a forward is an exchange: the ranks launch alike)
LAYOUTS = {"unequal": (40, 5), "empty": (40, 0)}


def _audience_case(rank, world, layout, excluded):
    import torch
    from tlsan_amd.dist import allgather_rows
    from tlsan_amd.model import SeenItems
    cfg = make_config(U=30, I=I, C=6, d=128)
    p = random_params(cfg, seed=91)
    p["item_b"][::3] = -0.0                                           # (a sum over the ranks would lose the sign)
    p["item_emb"][::5, ::3] = -0.0
    b, cat = random_batch(cfg, B=LAUNCH * world, Sn=3, seed=92, test=True)
    tb, _ = random_batch(cfg, B=16 * world, Sn=3, seed=93)
    sm = sharded(cfg, cat, p)                                         # lazy L2
    for _ in range(2):                                                # ... after two steps: the table scale is no longer 1
        sm.train(None, batch_tuple({k: v[rank * 16:(rank + 1) * 16] for k, v in tb.items()}), 1.0)
    assert float(sm._P.item()) != 1.0
    counts = LAYOUTS[layout][:world]
    real = counts[rank]
    part = batch_tuple({k: v[rank * LAUNCH:(rank + 1) * LAUNCH] for k, v in b.items()}, True)
    users = sm.user_vectors(part, real=[real])
    assert len(users) == real and users.row0 == sum(counts[:rank]) and users.n_total == sum(counts)
    items = np.array([0, 1, 2, 100, 255, 256, 7, 7, 128, 33, 64, 3, 9, 27, 81, 243, 0])       # both ranks' items, repeats
    # the parent's scorer on every rank's launch, gathered; the real rows in rank order are the global rows
    s = allgather_rows(sm.score_candidates(part, np.tile(items, (LAUNCH, 1))), sm.group).cpu().numpy()
    keep = np.concatenate([np.arange(r * LAUNCH, r * LAUNCH + counts[r]) for r in range(world)])
    s_all, u_all = s[keep], b["u"][keep]
    N = len(keep)
    rng = np.random.RandomState(94)                                   # (the same lists on every rank)
    lists = [rng.randint(-2, N + 3, q % 4 * 9) for q in range(len(items))]
    lists[1] = np.arange(N)                                           # every row: all -1 / -inf
    seen = [np.sort(rng.choice(I, rng.randint(0, 40), replace=False)) for _ in range(cfg["user_count"])]
    seen[int(u_all[0])] = np.union1d(seen[int(u_all[0])], [0, 7, 256])
    off, ids = np.cumsum([0] + [len(x) for x in seen]), np.concatenate(seen)
    forms = [(None, None)]
    if excluded:
        forms += [(lists, lists), (SeenItems(off, ids, sm.device), ref.seen_rows(off, ids, u_all, items))]
    for k in (1, 10, 64):
        for excl, gone in forms:
            rows, sc = [host(t) for t in sm.audience(items, k, users, exclude=excl)]
            want = ref.expected(s_all.T, k, gone)
            assert rows.dtype == np.int32 and np.array_equal(rows, want[0]), (k, gone is not None)
            assert np.array_equal(bits(sc), bits(want[1])), (k, gone is not None)
            who = host(users.users_of(rows))
            assert np.array_equal(who, np.where(rows >= 0, u_all[np.maximum(rows, 0)], -1))
    assert np.array_equal(rows[0], rows[-1]) and np.array_equal(rows[6], rows[7])             # the repeated items
    sm.train(None, batch_tuple({k: v[rank * 16:(rank + 1) * 16] for k, v in tb.items()}), 1.0)
    with pytest.raises(ValueError, match="rebuild"):
        sm.audience(items, 5, users)
    torch.cuda.synchronize()


@pytest.mark.parametrize("world,layout,excluded", [(1, "unequal", True), (2, "unequal", False), (2, "unequal", True),
                                                    (2, "empty", False)])
def test_sharded_audience_equals_the_gathered_scores_bit_for_bit(world, layout, excluded):
    run_ranks(_audience_case, world, layout, excluded)


def _sharded_driver_worker(rank, world, out):
    from tlsan_amd import train as T
    from tlsan_amd.input import seen_items_csr
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    train_set, test_set, (U, n_items, _), _ = T.load_dataset(ds)
    off, ids = seen_items_csr(train_set, U)
    busy = np.bincount(ids, minlength=n_items).argsort()[::-1][:2]
    items = [int(busy[0]), 0, int(busy[1])]
    T.train_sharded(T.parse(["--dataset", ds, "--max_steps", "5", "--eval_freq", "1000", "--quiet", "--train_batch_size", "33",
                             "--model_dir", os.path.join(out, "r%d" % rank), "--device_input", "0", "--l2_mode", "lazy",
                             "--audience_k", "5", "--audience_items", ",".join(map(str, items)), "--audience_exclude", "seen",
                             "--sharded", "1"]))
    path = os.path.join(out, "r%d" % rank, "audience-5.npz")
    assert os.path.exists(path) == (rank == 0)           # rank 0 writes
    if rank == 0:
        z = np.load(path)
        item, users, rows, sc = z["item"], z["users"], z["rows"], z["scores"]
        assert np.array_equal(item, items) and users.shape == rows.shape == sc.shape == (3, 5) and sc.dtype == np.float32
        assert rows.min() >= 0 and rows.max() < len(test_set) and all(len(set(x.tolist())) == 5 for x in rows)
        a, c = sc[:, :-1], sc[:, 1:]
        assert np.all((a > c) | ((a == c) & (rows[:, :-1] < rows[:, 1:])))
        for qi, it in enumerate(items):
            for u in users[qi]:
                assert 0 <= u < U and it not in ids[off[u]:off[u + 1]], (qi, it, u)


def test_sharded_driver_writes_audiences(tmp_path):
    run_ranks(_sharded_driver_worker, 2, str(tmp_path))

"""ShardedModel.recommend / similar_items with index= against Model's on the gathered parameters: the same ids and score
bits, with one rank and with two (two processes share cuda:0 and talk over gloo).  Every rank scans the lists of its own
item shard for all gathered rows; the unrestricted rows among them take the path without an index."""
import numpy as np
import pytest

from tests.helpers import batch_tuple, make_config, random_batch, random_params, sharded
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

I = 257                                                              # items not a multiple of the world size
ROWS = 22


def _same(got, want, what):
    got, want = [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want]
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), what
    return want


def _index_case(rank, world):
    from tlsan_amd.model import Model
    cfg = make_config(U=30, I=I, C=6, d=128)
    p = random_params(cfg, seed=81)
    p["item_emb"][::3, ::5] = -0.0                                   # (a sum over the ranks would lose the sign)
    b, cat = random_batch(cfg, B=ROWS * world, Sn=3, seed=82, test=True)
    cat[cat == 5] = 4                                                # category 5 is empty
    sm = sharded(cfg, cat, p, l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    part = batch_tuple({k: v[rank * ROWS:(rank + 1) * ROWS] for k, v in b.items()}, True)
    cate = m.last_item_categories(part).cpu().numpy().astype(np.int64)
    cate[rank::5] = -1                                               # unrestricted rows, other ones on every rank
    cate[(rank + 2) % 5::5] = 5
    probes = np.random.RandomState(7 + rank).randint(-1, 6, (ROWS, 3))
    probes[1] = -1
    probes[2] = [3, 3, -1]
    scope = np.arange(0, I, 3)
    for within in (None, scope):
        kw = {} if within is None else dict(within=sm.item_scope(items=within))
        si, mi = sm.category_index(**kw), m.category_index(**({} if within is None else dict(within=m.item_scope(items=within))))
        assert np.array_equal(si.list_off.cpu().numpy(), mi.list_off.cpu().numpy())
        assert np.array_equal(si.list_items.cpu().numpy(), mi.list_items.cpu().numpy()) and si.max_list == mi.max_list
        for k in (1, 10, 100):
            for extra in (dict(), dict(exclude="history")):
                want = _same(sm.recommend(part, k, category=cate, index=si, **extra),
                             m.recommend(part, k, category=cate, index=mi, **extra), (within is None, k, list(extra)))
                _same(sm.recommend(part, k, category=probes, index=si, **extra),
                      m.recommend(part, k, category=probes, index=mi, **extra), ("probes", within is None, k, list(extra)))
            assert (want[0][cate == 5] == -1).all()
        # ... and the sharded lists without the index
        _same(sm.recommend(part, 10, category=cate, index=si), sm.recommend(part, 10, category=cate, **kw), "no index")
        for extra in (dict(diversity=0.3, per_category=2, pool=64), dict(per_category=1, pool=32, exclude="history")):
            _same(sm.recommend(part, 10, category=cate, index=si, **extra), m.recommend(part, 10, category=cate, index=mi, **extra),
                  list(extra))
    si, mi = sm.category_index(), m.category_index()
    # similar_items is collective: every rank passes the same queries
    qids = np.array([0, 1, 2, 100, 255, 256, 7])
    for metric in ("cosine", "dot"):
        for extra in (dict(), dict(exclude=[[3, 6]] * len(qids))):
            for k in (5, 100):
                got = sm.similar_items(qids, k, metric=metric, same_category=True, index=si, **extra)
                _same(got, m.similar_items(qids, k, metric=metric, same_category=True, index=mi, **extra), (metric, list(extra), k))
                _same(sm.similar_items(qids, k, metric=metric, same_category=True, **extra), got, "no index")
    for kw in (dict(index=si), dict(index=si, category=cate, within=sm.item_scope(items=scope)), dict(index=si, category=np.full(ROWS, 6))):
        with pytest.raises(ValueError):
            sm.recommend(part, 10, **kw)
    with pytest.raises(ValueError):
        sm.similar_items(qids, 5, index=si)


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_indexed_lists_equal_the_model_bit_for_bit(world):
    run_ranks(_index_case, world)

"""ShardedModel.recommend with boost= / boost_weight= against Model's on the gathered parameters: the same ids and score
bits, with two ranks (two processes share cuda:0 and talk over gloo).  Every rank passes the same boost, indexed by global
id, and its own rows' weights; the weights are all-gathered with u_t and every rank scans its item shard with
(id_mul, id_add) = (world, rank)."""
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


def _boost_case(rank, world):
    from tlsan_amd.model import Model
    cfg = make_config(U=30, I=I, C=6, d=128)
    p = random_params(cfg, seed=91)
    b, cat = random_batch(cfg, B=ROWS * world, Sn=3, seed=92, test=True)
    sm = sharded(cfg, cat, p, l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    part = batch_tuple({k: v[rank * ROWS:(rank + 1) * ROWS] for k, v in b.items()}, True)
    rng = np.random.RandomState(5)                                   # every rank builds the same boost
    values = rng.randn(I).astype(np.float32)
    values[[0, 1, I - 1]] = 50.0                                     # lifted items on both shards, tied after the sum's rounding
    values[[2, 3, 100]] = -np.inf
    weights = np.random.RandomState(11 + rank).randn(ROWS).astype(np.float32)   # each rank's own rows
    weights[rank::4] = 0.0
    weights[(rank + 1) % 4::4] = 1.0
    sb, mb = sm.item_boost(values), m.item_boost(values)
    assert np.array_equal(sb.values.cpu().numpy(), mb.values.cpu().numpy())
    cate = m.last_item_categories(part).cpu().numpy().astype(np.int64)
    cate[rank::5] = -1
    probes = np.random.RandomState(7 + rank).randint(-1, 6, (ROWS, 3))
    probes[1] = -1                                                   # an unrestricted row: the sub-batch with its weight
    scope = np.arange(0, I, 3)
    ss, ms = sm.item_scope(items=scope), m.item_scope(items=scope)
    si, mi = sm.category_index(), m.category_index()
    moved = 0
    for k in (1, 10, 100):
        for w in (None, weights):
            bw = dict(boost_weight=w)
            want = _same(sm.recommend(part, k, boost=sb, **bw), m.recommend(part, k, boost=mb, **bw), ("plain", k, w is None))
            moved += int((want[0] != m.recommend(part, k)[0].cpu().numpy()).sum())
            _same(sm.recommend(part, k, boost=values, exclude="history", **bw), m.recommend(part, k, boost=mb, exclude="history", **bw),
                  ("history", k, w is None))
            _same(sm.recommend(part, k, boost=sb, within=ss, category=cate, **bw),
                  m.recommend(part, k, boost=mb, within=ms, category=cate, **bw), ("scoped", k, w is None))
            _same(sm.recommend(part, k, boost=sb, category=probes, index=si, **bw),
                  m.recommend(part, k, boost=mb, category=probes, index=mi, **bw), ("indexed", k, w is None))
    assert moved > 0
    _same(sm.recommend(part, 10, boost=sb, boost_weight=weights, diversity=0.3, per_category=2, pool=64),
          m.recommend(part, 10, boost=mb, boost_weight=weights, diversity=0.3, per_category=2, pool=64), "diversified")
    _same(sm.recommend(part, 10, boost=np.zeros(I, np.float32)), sm.recommend(part, 10), "a zero boost")
    for kw in (dict(boost_weight=weights), dict(boost=values[:-1]), dict(boost=sb, boost_weight=weights[:-1])):
        with pytest.raises(ValueError):
            sm.recommend(part, 10, **kw)


def test_sharded_boosted_lists_equal_the_model_bit_for_bit():
    run_ranks(_boost_case, 2)

"""ShardedModel.recommend with diversity / per_category against Model.recommend on the gathered parameters: the same ids
and score bits, with one rank and with two (two processes share cuda:0 and talk over gloo)."""
import numpy as np
import pytest

from tests.helpers import batch_tuple, make_config, random_batch, random_params, sharded
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu


def _rerank_case(rank, world):
    from tlsan_amd.model import Model
    cfg = make_config(U=30, I=257, C=6, d=128)                      # items not a multiple of the world size
    p = random_params(cfg, seed=81)
    p["item_emb"][::3, ::5] = -0.0                                   # (a sum over the ranks would lose the sign)
    b, cat = random_batch(cfg, B=22 * world, Sn=3, seed=82, test=True)
    sm = sharded(cfg, cat, p, l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    part = batch_tuple({k: v[rank * 22:(rank + 1) * 22] for k, v in b.items()}, True)
    for kw in (dict(diversity=0.5, per_category=2), dict(diversity=0.5, per_category=2, exclude="history", pool=256),
               dict(per_category=1, pool=16)):
        want = [t.cpu().numpy() for t in m.recommend(part, 10, **kw)]
        got = [t.cpu().numpy() for t in sm.recommend(part, 10, **kw)]
        assert got[0].shape == (22, 10) and np.array_equal(got[0], want[0]), kw
        assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), kw
    assert (want[0] < 0).any()                                       # 6 categories, one each: the rows end short
    plain = [t.cpu().numpy() for t in sm.recommend(part, 10)]
    again = [t.cpu().numpy() for t in sm.recommend(part, 10, diversity=0.0, per_category=0)]
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1].view(np.int32), again[1].view(np.int32))
    with pytest.raises(ValueError):
        sm.recommend(part, 10, pool=64)


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_diversified_recommend_equals_the_model_bit_for_bit(world):
    run_ranks(_rerank_case, world)

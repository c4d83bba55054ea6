"""ShardedModel.recommend with diversity / per_category against Model.recommend on the gathered parameters: the same ids
and score bits, with one rank and with two (two processes share cuda:0 and talk over gloo)."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import make_config, random_batch, random_params
from tests.test_gpu_dist import _free_port
from tests.test_gpu_dist_lazy_opt import _sharded

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, ret, name, *args):
    """globals()[name](rank, world, *args) inside a gloo group, its outcome in ret[rank]"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        globals()[name](rank, world, *args)
        ret[rank] = "ok"
    except Exception:
        import traceback
        ret[rank] = "FAIL: " + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def _spawn(fn, world, *args):
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), ret, fn.__name__) + args, nprocs=world, join=True)
    assert all(v == "ok" for v in dict(ret).values()) and len(ret) == world, dict(ret)


def _tuple(b):
    return (b["u"], b["i"], b["j"], b["hist_i"], b["hist_i_new"], b["hist_t"], b["sl"], b["sl_new"], b["u_cate"])


def _rerank_case(rank, world):
    from tlsan_amd.model import Model
    cfg = make_config(U=30, I=257, C=6, d=128)                      # items not a multiple of the world size
    p = random_params(cfg, seed=81)
    p["item_emb"][::3, ::5] = -0.0                                   # (a sum over the ranks would lose the sign)
    b, cat = random_batch(cfg, B=22 * world, Sn=3, seed=82, test=True)
    sm = _sharded(cfg, cat, p, l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    part = _tuple({k: v[rank * 22:(rank + 1) * 22] for k, v in b.items()})
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
    _spawn(_rerank_case, world)

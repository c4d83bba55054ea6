"""ShardedModel.list_metrics against Model.list_metrics on the gathered parameters: the same bits in all seven outputs, and
exposure counters that add up over the ranks -- with one rank and with two (two processes share cuda:0 and talk over
gloo).  The fixture of tests/test_gpu_dist_rerank.py."""
import numpy as np
import pytest

from tests.helpers import batch_tuple, make_config, random_batch, random_params, sharded
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu


def _list_metrics_case(rank, world):
    import torch
    from tlsan_amd.dist import allreduce_sum
    from tlsan_amd.model import Model
    I = 257                                                          # items not a multiple of the world size
    cfg = make_config(U=30, I=I, C=6, d=128)
    p = random_params(cfg, seed=81)
    p["item_emb"][::3, ::5] = -0.0                                   # (a sum over the ranks would lose the sign)
    b, cat = random_batch(cfg, B=22 * world, Sn=3, seed=82, test=True)
    sm = sharded(cfg, cat, p, l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    mine = slice(rank * 22, (rank + 1) * 22)
    part = batch_tuple({k: v[mine] for k, v in b.items()}, True)
    weight = (np.random.RandomState(9).rand(I) * 7).astype(np.float32)
    ids = sm.recommend(part, 10, diversity=0.5, per_category=2)[0]
    ids[3, 4] = -1                                                   # a hole, which recommend never makes
    expo_s = torch.zeros(I, dtype=torch.int32, device=sm.device)
    expo_m = torch.zeros(I, dtype=torch.int32, device=m.device)
    got = sm.list_metrics(ids, labels=b["i"][mine], item_weight=weight, exposure=expo_s)
    want = m.list_metrics(ids.clone(), labels=b["i"][mine], item_weight=weight, exposure=expo_m)
    for name, g, w in zip(got._fields, got, want):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        assert g.shape == (22,) and g.dtype == w.dtype, name
        as_int = lambda x: x.view(np.int64) if x.dtype == np.float64 else x
        assert np.array_equal(as_int(g), as_int(w)), name            # (pair_cos, ild, weight_sum: compared as int64 bits)
    valid = (ids.cpu().numpy() >= 0).sum(1)
    assert np.array_equal(got.n.cpu().numpy(), valid), (got.n.cpu().numpy(), valid)
    assert valid[3] <= 9 and valid.min() >= 2, valid
    assert (got.max_cate.cpu().numpy() <= 2).all() and (got.max_cate.cpu().numpy() == 2).any()
    assert torch.equal(expo_s, expo_m)
    # the ranks' counters add up to the single model's over all rows
    all_ids = m.recommend(batch_tuple(b, True), 10, diversity=0.5, per_category=2)[0]
    all_ids[[r * 22 + 3 for r in range(world)], 4] = -1               # (every rank made that hole in its rows)
    expo_all = torch.zeros(I, dtype=torch.int32, device=m.device)
    m.list_metrics(all_ids, exposure=expo_all)
    total = expo_s.to(torch.int64)
    if world > 1:
        total = allreduce_sum(total, sm.group)
    assert torch.equal(total, expo_all.to(torch.int64)) and int(total.sum()) == int((all_ids >= 0).sum()) > 0
    with pytest.raises(ValueError):
        sm.list_metrics(ids, labels=b["i"][:5])                      # (refused on every rank, before anything collective)


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_list_metrics_equal_the_model_bit_for_bit(world):
    run_ranks(_list_metrics_case, world)

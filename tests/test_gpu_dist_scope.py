"""ShardedModel.recommend / similar_items with within= / category= / same_category= against Model's on the gathered
parameters: the same ids and score bits, with one rank and with two (two processes share cuda:0 and talk over gloo)."""
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


def _scope_case(rank, world):
    from tlsan_amd.model import Model
    cfg = make_config(U=30, I=I, C=6, d=128)
    p = random_params(cfg, seed=81)
    p["item_emb"][::3, ::5] = -0.0                                   # (a sum over the ranks would lose the sign)
    b, cat = random_batch(cfg, B=ROWS * world, Sn=3, seed=82, test=True)
    sm = sharded(cfg, cat, p, l2_mode="dense")
    m = Model(cfg, cat)
    m.set_params({k: np.asarray(v, np.float32) for k, v in sm.gather_params().items()})
    part = batch_tuple({k: v[rank * ROWS:(rank + 1) * ROWS] for k, v in b.items()}, True)
    cate = m.last_item_categories(part)
    assert np.array_equal(sm.last_item_categories(part).cpu().numpy(), cate.cpu().numpy())
    scopes = dict(A=np.arange(0, I, 3), odd=np.arange(1, I, 2),      # odd: with two ranks, entirely on rank 1
                  few=np.array([0, 5, 256]), none=np.zeros(0, np.int64), cate=None)
    for name, ids in scopes.items():
        kw = dict(categories=[1, 4]) if ids is None else dict(items=ids)
        ws, wm = sm.item_scope(**kw), m.item_scope(**kw)
        assert np.array_equal(ws.ids.cpu().numpy(), wm.ids.cpu().numpy()), name
        for k in (1, 10, 100):
            for extra in (dict(), dict(category=cate), dict(category=cate, exclude="history")):
                want = _same(sm.recommend(part, k, within=ws, **extra), m.recommend(part, k, within=wm, **extra), (name, k, list(extra)))
        if name == "few":
            assert (want[0][:, 3:] == -1).all()
    for k in (1, 10):                                                # the category alone
        _same(sm.recommend(part, k, category=cate), m.recommend(part, k, category=cate), ("C", k))
    ws, wm = sm.item_scope(items=scopes["A"]), m.item_scope(items=scopes["A"])
    for kw in (dict(diversity=0.3, per_category=2, pool=64), dict(per_category=1, pool=32, category=cate),
               dict(diversity=0.5, exclude="history")):
        _same(sm.recommend(part, 10, within=ws, **kw), m.recommend(part, 10, within=wm, **kw), list(kw))
    plain = sm.recommend(part, 10)                                   # with neither, nothing changes
    _same(sm.recommend(part, 10, within=None, category=None), plain, "plain")
    # similar_items is collective: every rank passes the same queries
    qids = np.array([0, 1, 2, 100, 255, 256, 7])
    os_, om = sm.item_scope(items=scopes["odd"]), m.item_scope(items=scopes["odd"])
    for metric in ("cosine", "dot"):
        for ks, km in ((dict(same_category=True), dict(same_category=True)), (dict(within=ws), dict(within=wm)),
                       (dict(within=os_, same_category=True), dict(within=om, same_category=True)),
                       (dict(within=ws, exclude=[[3, 6]] * len(qids)), dict(within=wm, exclude=[[3, 6]] * len(qids)))):
            for k in (5, 100):
                _same(sm.similar_items(qids, k, metric=metric, **ks), m.similar_items(qids, k, metric=metric, **km),
                      (metric, list(ks), k))
    with pytest.raises(ValueError):
        sm.recommend(part, 10, category=np.full(ROWS, 6))
    with pytest.raises(ValueError):
        sm.recommend(part, 10, within=[1, 2])


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_scoped_lists_equal_the_model_bit_for_bit(world):
    run_ranks(_scope_case, world)

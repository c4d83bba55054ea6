"""GPU parity tests: the HIP path (through the C ABI, via tlsan_amd.Model) against the CPU
oracle on the same seeded inputs.  Tolerances: fp32 logits within 1e-4 of the fp64 oracle
(BASELINE.json north_star); gradients / updated parameters within 2e-4 relative to the tensor's
max magnitude (fp32 accumulation order differs); index/mask behaviour exact."""
import os

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.helpers import (BF16_TABLES, batch_tuple, bf16_round, fixture_batch, make_config, model, p32, random_batch,
                           random_params)

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4


def _relerr(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-12)


@pytest.mark.parametrize("d,B,Sn", [(64, 37, 3), (128, 50, 5), (128, 16, 0), (128, 1, 2), (256, 21, 4),
                                    (64, 200, 12), (128, 300, 18)])
def test_forward_logits(d, B, Sn):
    cfg = make_config(U=70, I=90, C=11, d=d)
    p = p32(random_params(cfg, seed=d + B))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=B + Sn, test=True)
    m = model(cfg, cat, p)
    li, lj, ut, _ = m.forward(batch_tuple(b, True), is_test=True, want_u_t=True)
    ref = orc.forward(p, cat, b, 8)
    bn = dict(b); bn["i"] = b["j"]
    refj = orc.forward(p, cat, bn, 8)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    assert np.abs(lj.cpu().numpy() - refj["logits"]).max() < LOGIT_TOL
    assert np.abs(ut.cpu().numpy() - ref["u_t"]).max() < LOGIT_TOL
    auc = m.eval_auc(None, batch_tuple(b, True))
    assert auc == pytest.approx(float(np.mean(ref["logits"] - refj["logits"] > 0)), abs=1e-6)


@pytest.mark.parametrize("d,B,Sn", [(64, 45, 4), (128, 40, 3), (128, 33, 9), (256, 18, 2), (128, 1, 0)])
def test_gradients(d, B, Sn):
    cfg = make_config(U=30, I=50, C=7, d=d)  # small tables -> many duplicate ids
    p = p32(random_params(cfg, seed=3 * d + B))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=B * 7 + Sn)
    reg = cfg["regulation_rate"]
    loss, logits, g, sparse = orc.backward(p, cat, b, 8, reg)
    m = model(cfg, cat, p)
    out = m.grads(batch_tuple(b))
    assert np.abs(out["logits"] - logits).max() < LOGIT_TOL
    assert abs(out["loss"] - loss) < 1e-4 * max(1.0, abs(loss))
    for k in g:
        gk = np.asarray(out["grads"][k], np.float64).reshape(g[k].shape)
        # absolute floor: d/d b2 is identically 0 (softmax is shift invariant), fp32 leaves ~1e-9
        err = np.abs(gk - g[k]).max()
        assert err < 2e-4 * np.abs(g[k]).max() + 1e-6, (k, err, np.abs(g[k]).max())
    n18 = orc.global_norm(p, g, sparse, reg, "tf18")
    assert abs(out["gnorm"] - n18) < 2e-4 * n18
    m2 = model(cfg, cat, p, norm_mode="dedup")
    out2 = m2.grads(batch_tuple(b))
    nd = orc.global_norm(p, g, sparse, reg, "dedup")
    assert abs(out2["gnorm"] - nd) < 2e-4 * nd


@pytest.mark.parametrize("norm_mode", ["tf18", "dedup"])
@pytest.mark.parametrize("clip", [5.0, 0.02])
def test_train_step_matches_oracle(norm_mode, clip):
    cfg = make_config(U=40, I=60, C=9, d=128, max_gradient_norm=clip, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=11))
    b, cat = random_batch(cfg, B=48, Sn=4, seed=12)
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.7, clip=clip,
                                      norm_mode=norm_mode)
    if clip < 1:
        assert info["coef"] < 1.0
    m = model(cfg, cat, p, norm_mode=norm_mode)
    l = m.train(None, batch_tuple(b), 0.7)
    assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
    got = m.get_params()
    for k in newp:
        # compare the UPDATE (new - old), which is what the kernels compute
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < 2e-4 * (np.abs(dr).max() + 1e-9) + 2e-7, k
    # K^T copy is kept in sync
    assert np.array_equal(m.dense_KT.cpu().numpy(), got["dense_K"].T)


@pytest.mark.parametrize("d,Ls,l2_mode", [(128, 10, "dense"), (128, 10, "lazy"), (64, 10, "lazy"), (128, 24, "lazy"), (256, 16, "dense")])
def test_category_segments_match_oracle(d, Ls, l2_mode):
    """Many categories (>= 2048, BASELINE.json configs[4] has 10 k): the category half of every item use's gradient row is
    written into the category's own segment (FwdArgs.cseg / ApplyArgs.cseg) instead of beside the item half, and the
    category blocks of the apply pass sum that segment instead of walking the category's items.  Same numbers as the
    oracle: gradients, three training steps (window in registers and streamed, dense and lazy L2), bitwise reproducible."""
    cfg = make_config(U=70, I=2600, C=2100, d=d, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=91))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=41, Sn=2 + s, seed=900 + s)[0] for s in range(3)]
    for b in batches:          # (several uses per item and per category: ids folded onto 150 items; u_cate hits their categories)
        for k in ("hist_i", "hist_i_new", "i"):
            b[k] %= 150
        b["u_cate"][:] = cat[b["i"]]
    m = model(cfg, cat, p, l2_mode=l2_mode)
    g = m.grads(batch_tuple(batches[0]))
    _, _, ref_g, _ = orc.backward(p, cat, batches[0], 8, cfg["regulation_rate"])
    for k in ref_g:
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.abs(a - r).max() < 2e-4 * np.abs(r).max() + 1e-6, k
    runs = []
    for rep in range(2):
        mm = model(cfg, cat, p, l2_mode=l2_mode)
        losses = [mm.train(None, batch_tuple(b), 0.6) for b in batches]
        runs.append((losses, mm.get_params()))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
    q = dict(p)
    for b, l in zip(batches, runs[0][0]):
        lo, q, _ = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=0.6)
        assert abs(l - lo) < 2e-4 * max(1.0, abs(lo))
    for k in q:
        du = np.asarray(runs[0][1][k], np.float64).reshape(p[k].shape) - p[k]
        dr = q[k] - p[k]
        assert np.abs(du - dr).max() < 5e-4 * (np.abs(dr).max() + 1e-9) + 5e-7, k


def test_category_segments_with_many_uses_per_category():
    """Category segments with MORE than 512 uses per category (2 100 categories, 12 000 samples, a 90-slot streamed
    window: 543 uses each) -- the shape at which the row-sum pass of the item-walk path splits a category over several
    workgroups.  A category segment is never split (round 3's advisor: `category_split` ran with `cseg` set and the
    split kernel then summed the first C/16 categories only, silently): one lazy step against the oracle."""
    cfg = make_config(U=70, I=2600, C=2100, d=64, Ls=90, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=93))
    b, cat = random_batch(cfg, B=12000, Sn=3, seed=931)
    assert b["u"].shape[0] * (cfg["Ls"] + 3 + 2) // cfg["cate_count"] > 512
    m = model(cfg, cat, p, l2_mode="lazy")
    loss = m.train(None, batch_tuple(b), 0.6)
    lo, q, _ = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.6)
    assert abs(loss - lo) < 2e-4 * max(1.0, abs(lo))
    got = m.get_params()
    for k in q:
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = q[k] - p[k]
        assert np.abs(du - dr).max() < 5e-4 * (np.abs(dr).max() + 1e-9) + 5e-7, k


def test_multi_step_tracks_oracle_and_is_deterministic():
    cfg = make_config(U=25, I=35, C=5, d=64, regulation_rate=5e-5)
    p = p32(random_params(cfg, seed=21))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=40, Sn=1 + s % 4, seed=100 + s)[0] for s in range(6)]
    runs = []
    for rep in range(2):
        m = model(cfg, cat, p)
        losses = [m.train(None, batch_tuple(b), 0.5) for b in batches]
        runs.append((losses, m.get_params()))
    # bitwise reproducible (deterministic scatter-add and reductions)
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
    q = dict(p)
    ref_losses = []
    for b in batches:
        l, q, _ = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=0.5)
        ref_losses.append(l)
    assert np.allclose(runs[0][0], ref_losses, rtol=2e-4, atol=1e-5)
    for k in q:
        got = np.asarray(runs[0][1][k], np.float64).reshape(q[k].shape)
        assert np.abs(got - q[k]).max() < 5e-4 * np.abs(q[k]).max() + 1e-6, k


@pytest.mark.parametrize("name", ["clothing", "digital_music"])
def test_real_fixture_batches(name):
    """Real batches from the reference's input.py, reference default shapes (d=64, B=32/128)."""
    batch, (U, I, C), icl = fixture_batch(name)
    cfg = make_config(U=U, I=I, C=C, d=64)
    p = p32(orc.init_params(cfg, seed=1234))
    rng = np.random.RandomState(5)
    p["item_b"] = rng.uniform(-0.1, 0.1, p["item_b"].shape).astype(np.float32).astype(np.float64)
    m = model(cfg, icl, p)
    b = orc.as_batch(batch)
    loss, newp, info = orc.train_step(p, icl, b, 8, cfg["regulation_rate"], 1.0)
    l = m.train(None, batch, 1.0)
    assert abs(l - loss) < 1e-4 * max(1.0, loss)
    got = m.get_params()
    for k in newp:
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 2e-7, k
    tb, _, _ = fixture_batch(name, "DataInputTest", 128, 10, 0)
    tbd = orc.as_batch(tb, is_test=True)
    q = p32(got)
    auc_ref, r1, r2 = orc.eval_auc_batch(q, icl, tbd, 8)
    assert m.eval_auc(None, tb) == pytest.approx(auc_ref, abs=1.0 / 128 + 1e-9)
    li, lj, _, _ = m.forward(tb, is_test=True)
    assert np.abs(li.cpu().numpy() - r1).max() < LOGIT_TOL


@pytest.mark.parametrize("d", [64, 128])
def test_eval_ranks_and_metrics(d):
    cfg = make_config(U=60, I=333, C=13, d=d)
    p = p32(random_params(cfg, seed=31))
    b, cat = random_batch(cfg, B=77, Sn=3, seed=32, test=True)
    m = model(cfg, cat, p)
    ranks = m.label_ranks(batch_tuple(b, True)).cpu().numpy()
    ref = orc.forward(p, cat, b, 8)
    scores = orc.all_item_scores(p, cat, ref["u_t"])
    rr = orc.label_ranks(scores, b["i"])
    # fp32 scores vs fp64 oracle: ranks may differ only where two scores are within rounding
    srt = np.sort(scores, axis=1)
    gap = np.abs(scores[np.arange(len(rr)), b["i"]][:, None] - scores)
    gap[np.arange(len(rr)), b["i"]] = np.inf
    clear = gap.min(1) > 1e-4
    assert clear.sum() > 60
    assert np.array_equal(ranks[clear], rr[clear])
    assert np.abs(ranks - rr).max() <= 2
    pr = m.eval_prec(None, batch_tuple(b, True))
    rc = m.eval_recall(None, batch_tuple(b, True))
    hits = orc.hits_at_k(scores, b["i"])
    for i, k in enumerate((1, 10, 20, 30, 40, 50)):
        assert abs(pr[i] - hits[i] / (k * 77)) <= 2 / (k * 77) + 1e-9
        assert abs(rc[i] - hits[i] / 77) <= 2 / 77 + 1e-9
    # cumulative semantics (reference never resets the streaming counters)
    pr2 = m.eval_prec(None, batch_tuple(b, True))
    assert np.allclose(pr2, pr)
    assert m.prec_10.eval() == pytest.approx(pr2[1])


def test_exact_ties_follow_topk_order():
    """Two items with bit-identical rows and biases: the lower id ranks first (tf.nn.top_k)."""
    cfg = make_config(U=20, I=64, C=4, d=64)
    p = p32(random_params(cfg, seed=41))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=42, test=True)
    p["item_emb"][9] = p["item_emb"][5]
    p["item_b"][9] = p["item_b"][5]
    cat[9] = cat[5]
    b["i"][:8] = 5
    b["i"][8:] = 9
    m = model(cfg, cat, p)
    ranks = m.label_ranks(batch_tuple(b, True)).cpu().numpy()
    ref = orc.forward(p, cat, b, 8)
    scores = orc.all_item_scores(p, cat, ref["u_t"]).astype(np.float32)
    # label 9 must count item 5 as ahead of it, label 5 must not count item 9
    m2 = model(cfg, cat, p)
    b2 = dict(b); b2["i"] = np.where(b["i"] == 5, 9, 5)
    ranks2 = m2.label_ranks(batch_tuple(b2, True)).cpu().numpy()
    assert np.array_equal(ranks2[:8], ranks[:8] + 1)
    assert np.array_equal(ranks2[8:], ranks[8:] - 1)


def test_errors():
    from tlsan_amd.model import Model
    from tlsan_amd._lib import TlsanError
    cfg = make_config(d=96)
    with pytest.raises(TlsanError):
        Model(cfg, np.zeros(cfg["item_count"], np.int32))
    cfg = make_config(d=64, optimizer="adagrad")          # not one of model.py:188-195
    with pytest.raises(ValueError):
        Model(cfg, np.zeros(cfg["item_count"], np.int32))
    cfg = make_config(d=64)
    m = Model(cfg, np.zeros(cfg["item_count"], np.int32))
    b, _ = random_batch(cfg, B=4, Sn=2, seed=1)
    bad = list(batch_tuple(b)); bad[3] = bad[3][:, :5]
    with pytest.raises(ValueError):
        m.train(None, tuple(bad), 1.0)


@pytest.mark.parametrize("clip", [5.0, 0.02])
def test_lazy_l2_matches_dense_oracle(clip):
    """l2_mode='lazy' (scaled representation, only used rows touched) is the reference's dense-L2
    update up to fp32 rounding: several steps against the (dense) oracle, clip active and not."""
    cfg = make_config(U=300, I=200, C=9, d=128, max_gradient_norm=clip, regulation_rate=2e-2)  # big reg: decay visible
    p = p32(random_params(cfg, seed=51))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=24, Sn=1 + s % 3, seed=300 + s)[0] for s in range(5)]
    m = model(cfg, cat, p, l2_mode="lazy")
    q = dict(p)
    for b in batches:
        l = m.train(None, batch_tuple(b), 0.9)
        lo, q, info = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=0.9, clip=clip)
        assert abs(l - lo) < 2e-4 * max(1.0, abs(lo))
        assert abs(m.last_gnorm() - info["norm"]) < 3e-4 * info["norm"]
    P = m.table_scale()
    assert P < (0.95 if clip > 1 else 1.0)  # the decay really lives in the scale
    # evaluation uses the scale on the fly
    tb, _ = random_batch(cfg, B=20, Sn=2, seed=99, test=True)
    li, lj, ut, _ = m.forward(batch_tuple(tb, True), is_test=True, want_u_t=True)
    ref = orc.forward(q, cat, tb, 8)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < 3e-4
    ranks = m.label_ranks(batch_tuple(tb, True)).cpu().numpy()
    rr = orc.label_ranks(orc.all_item_scores(q, cat, ref["u_t"]), tb["i"])
    assert np.abs(ranks - rr).max() <= 2
    got = m.get_params()  # folds the scale
    assert m.table_scale() == 1.0
    for k in q:
        g = np.asarray(got[k], np.float64).reshape(q[k].shape)
        assert np.abs(g - q[k]).max() < 5e-4 * np.abs(q[k]).max() + 1e-6, k
    # training continues correctly after the fold
    b = batches[0]
    l = m.train(None, batch_tuple(b), 0.9)
    lo, q, _ = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=0.9, clip=clip)
    assert abs(l - lo) < 2e-4 * max(1.0, abs(lo))


def test_lazy_is_deterministic_and_untouched_rows_are_not_written():
    cfg = make_config(U=400, I=300, C=7, d=64, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=61))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=62)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, l2_mode="lazy")
        before = m.user_emb.clone()
        m.train(None, batch_tuple(b), 1.0)
        touched = np.zeros(cfg["user_count"], bool)
        touched[b["u"]] = True
        same = (m.user_emb == before).all(dim=1).cpu().numpy()
        assert same[~touched].all() and not same[touched].any()
        outs.append(m.get_params())
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_long_sessions_and_short_window():
    """Sessions longer than one prefetch chunk (32 ids at d=128, 16 at d=64) and Ls < 10."""
    for d, Ls, Sn in ((128, 6, 40), (64, 4, 37), (128, 10, 70)):
        cfg = make_config(U=40, I=120, C=6, d=d, Ls=Ls)
        p = p32(random_params(cfg, seed=d + Sn))
        b, cat = random_batch(cfg, B=19, Sn=Sn, seed=Sn)
        b["sl_new"][:3] = [Sn, Sn - 1, 33 if Sn > 33 else Sn]
        ar = np.arange(Sn)[None, :]
        rng = np.random.RandomState(1)
        b["hist_i_new"] = np.where(ar < b["sl_new"][:, None], rng.randint(0, 120, (19, Sn)), 0)
        loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.5)
        for l2 in ("dense", "lazy"):
            m = model(cfg, cat, p, l2_mode=l2)
            l = m.train(None, batch_tuple(b), 0.5)
            assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (d, Ls, Sn, l2)
            got = m.get_params()
            for k in newp:
                du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
                dr = newp[k] - p[k]
                assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 5e-7, (k, d, Ls, Sn, l2)
    # sessions beyond the documented cap are rejected, not mis-computed
    from tlsan_amd._lib import TlsanError
    cfg = make_config(U=10, I=20, C=3, d=64)
    b, cat = random_batch(cfg, B=4, Sn=100, seed=1)
    m = model(cfg, cat)
    with pytest.raises(TlsanError):
        m.train(None, batch_tuple(b), 1.0)


def test_graph_replay_equals_eager():
    cfg = make_config(U=200, I=150, C=9, d=128)
    p = p32(random_params(cfg, seed=71))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=64, Sn=3, seed=400 + s)[0] for s in range(3)]
    outs = []
    for mode in ("eager", "graph"):
        m = model(cfg, cat, p, l2_mode="lazy")
        if mode == "graph":
            graphs = [m.capture_step(batch_tuple(b), 0.7) for b in batches]
            # capture_step runs one warm step per batch: rebuild the same starting point
            m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
            for rep in range(2):
                for g in graphs:
                    m.replay(g)
        else:
            for rep in range(2):
                for b in batches:
                    m.train_async(batch_tuple(b), 0.7)
        outs.append(m.get_params())
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("C,l2_mode", [(40, "lazy"), (3, "lazy"), (3, "dense")])
def test_full_size_batch_matches_oracle(C, l2_mode):
    """One step at the bench shape class (B=4096 -> 256 workgroup passes, hot rows, hot categories).
    C=3: ~13k uses and ~670 items per category -> the category blocks of k_apply take several
    256-item passes and the segment-by-segment path (use list larger than AP_CAP)."""
    from tlsan_amd import synth
    cfg = synth.make_config("electronics", user_count=3000, item_count=2000, cate_count=C)
    icl = synth.item_cate_list(cfg)
    batch = synth.make_batches(cfg, 1, 4096, seed=5)[0]
    m = model(cfg, icl, l2_mode=l2_mode)
    p = {k: np.asarray(v, np.float64) for k, v in m.get_params().items()}
    b = orc.as_batch(batch)
    loss, newp, info = orc.train_step(p, icl, b, 8, cfg["regulation_rate"], lr=1.0)
    l = m.train(None, batch, 1.0)
    assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
    got = m.get_params()
    for k in newp:
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 5e-7, k


def test_train_driver_on_real_clothing(tmp_path):
    """tlsan_amd.train (the reference's train.py flow) on the real Clothing tuples: AUC must rise
    from its initial value within 600 steps at the reference's hyper-parameters."""
    import os
    from tlsan_amd import train as T
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    res = T.train(T.parse(["--dataset", ds, "--max_steps", "600", "--eval_freq", "300", "--quiet",
                           "--model_dir", str(tmp_path / "ckpt")]))
    assert res["steps"] == 600
    assert 0.80 < res["init_auc"] < 0.90          # the README leak quirk: ~0.86 at random init
    assert res["final_auc"] > res["init_auc"] + 0.003
    assert len(res["prec"]) == 6 and 0.0 <= res["recall"][-1] <= 1.0
    # summaries (model.py:174-183, train.py:91-118) land next to the checkpoints as step,tag,value rows
    rows = [l.strip().split(",") for l in open(tmp_path / "ckpt" / "train" / "scalars.csv")]
    tags = {r[1] for r in rows}
    assert {"Training Loss", "L2_norm_user_item", "gamma", "embedding/1_item_emb/std"} <= tags
    assert sorted({int(r[0]) for r in rows}) == [100, 200, 300, 400, 500, 600]          # display_freq 100
    ev = [l.strip().split(",") for l in open(tmp_path / "ckpt" / "eval" / "scalars.csv")]
    assert [float(r[2]) for r in ev if r[1] == "AUC"][-1] == pytest.approx(res["final_auc"], abs=1e-6)
    assert {"P@1", "P@50", "R@20"} <= {r[1] for r in ev}


def test_chunked_evaluation_equals_the_reference_batches():
    """The driver evaluates in launches of train.EVAL_CHUNK rows and forms the reference's per-batch aggregation
    (train.py:86-118, test batch 128) from slices of the per-row results: same AUC, same cumulative P@k / R@k
    counters as feeding the kernels 128 rows at a time."""
    import os
    from tlsan_amd import train as T
    from tlsan_amd.input import DataInputTest, load_packed
    from tlsan_amd.model import KS, Model
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    _, test_set, (U, I, Cc), icl = load_packed(ds)
    cfg = {n: d for n, _, d in T.FLAGS}
    cfg.update(user_count=U, item_count=I, cate_count=Cc, quiet=True)
    a, b = Model(cfg, icl, seed=3), Model(cfg, icl, seed=3)
    assert len(test_set) > T.EVAL_CHUNK // 4
    for rounds in range(2):                              # (the counters are cumulative: two evaluation rounds)
        auc_a = T.eval_auc(a, test_set, cfg)
        pa, ra = T.eval_prec_recall(a, test_set, cfg)
        s = 0.0
        for _, batch in DataInputTest(test_set, cfg["test_batch_size"], cfg["Ls"]):
            s += b.eval_auc(None, batch) * len(batch[0])
        auc_b = s / len(test_set)
        for _, batch in DataInputTest(test_set, cfg["test_batch_size"], cfg["Ls"]):
            b.eval_prec(None, batch)
        pb = [getattr(b, "prec_%d" % k).eval() for k in KS]
        for _, batch in DataInputTest(test_set, cfg["test_batch_size"], cfg["Ls"]):
            b.eval_recall(None, batch)
        rb = [getattr(b, "recall_%d" % k).eval() for k in KS]
        assert auc_a == auc_b
        assert list(pa) == list(pb) and list(ra) == list(rb)


@pytest.mark.parametrize("d,Ls,Sn,B", [(128, 20, 3, 37), (128, 90, 5, 21), (64, 33, 2, 50), (256, 16, 2, 9), (256, 90, 4, 19),
                                       (128, 40, 3, 300), (64, 90, 2, 131), (256, 33, 2, 70), (256, 90, 4, 150)])
def test_long_windows_streamed(d, Ls, Sn, B):
    """Ls > 10 (BASELINE configs 3/4: seq <= 90): the long block is streamed with an online
    softmax; forward, one training step (dense and lazy L2) and eval against the oracle.
    (The larger batches: several workgroup passes, a last one that is not full, the samples ranked by window length and
    dealt out to the passes, each pass's windows walked as one list whose runs are merged through the LDS.)"""
    cfg = make_config(U=50, I=150, C=8, d=d, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=Ls + d))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=Ls)
    b["sl"][:4] = [Ls, 1, Ls - 1, min(Ls, 11)]
    ar = np.arange(Ls)[None, :]
    b["hist_i"] = np.where(ar < b["sl"][:, None], np.random.RandomState(2).randint(0, 150, (B, Ls)), 0)
    b["hist_t"] = np.where(ar < b["sl"][:, None], (1.0 / np.random.RandomState(3).randint(1, 13, (B, Ls))), 0).astype(np.float32)
    ref = orc.forward(p, cat, b, 8)
    m0 = model(cfg, cat, p)
    tb = dict(b); tb["j"] = b["i"][::-1].copy()
    li, lj, ut, _ = m0.forward(batch_tuple(tb, True), is_test=True, want_u_t=True)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    assert np.abs(ut.cpu().numpy() - ref["u_t"]).max() < LOGIT_TOL
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.6)
    for l2 in ("dense", "lazy"):
        m = model(cfg, cat, p, l2_mode=l2)
        l = m.train(None, batch_tuple(b), 0.6)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), l2
        assert abs(m.last_gnorm() - info["norm"]) < 3e-4 * info["norm"], l2
        got = m.get_params()
        for k in newp:
            du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
            dr = newp[k] - p[k]
            assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 5e-7, (k, l2)


@pytest.mark.parametrize("d,Ls,Sn,B", [(128, 20, 3, 37), (128, 90, 5, 21), (64, 33, 2, 50)])
def test_bf16_tables_with_streamed_windows(d, Ls, Sn, B):
    """bf16 table storage with Ls > 10 (the Movies-TV configuration asks for both): forward and gradients equal the
    fp64 oracle evaluated on the stored (bf16-rounded) tables, and a training step runs and is reproducible."""
    cfg = make_config(U=50, I=150, C=8, d=d, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=Ls + d))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=Ls)
    b["sl"][:4] = [Ls, 1, Ls - 1, min(Ls, 11)]
    ar = np.arange(Ls)[None, :]
    b["hist_i"] = np.where(ar < b["sl"][:, None], np.random.RandomState(2).randint(0, 150, (B, Ls)), 0)
    b["hist_t"] = np.where(ar < b["sl"][:, None], (1.0 / np.random.RandomState(3).randint(1, 13, (B, Ls))), 0).astype(np.float32)
    m = model(cfg, cat, p, l2_mode="lazy", table_dtype="bf16")
    ref = orc.forward(p, cat, b, 8)
    li, _, _, _ = m.forward(batch_tuple(b), is_test=False)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    g = m.grads(batch_tuple(b))
    _, _, ref_g, _ = orc.backward(p, cat, b, 8, cfg["regulation_rate"])
    for k in ref_g:
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.abs(a - r).max() < 3e-4 * np.abs(r).max() + 1e-6, k
    loss = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.6)[0]
    outs = []
    for rep in range(2):
        mm = model(cfg, cat, p, l2_mode="lazy", table_dtype="bf16")
        l = mm.train(None, batch_tuple(b), 0.6)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        outs.append(mm.get_params())
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


_BF16_CLIP_DUMP = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tests.helpers import BF16_TABLES, batch_tuple, bf16_round, make_config, p32, random_batch, random_params
from tlsan_amd.model import Model
cfg = make_config(U=40, I=60, C=9, d=128, max_gradient_norm=0.02, regulation_rate=1e-3)
p = p32(random_params(cfg, seed=41))
for k in BF16_TABLES:
    p[k] = bf16_round(p[k]).astype(np.float64)
b, cat = random_batch(cfg, B=48, Sn=4, seed=42)
m = Model(cfg, cat, l2_mode="lazy", table_dtype="bf16")
m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
loss = m.train(None, batch_tuple(b), 0.7)
np.savez(sys.argv[1], loss=loss, gnorm=m.last_gnorm(), **m.get_params())
'''


def test_bf16_tables_clipped_step_in_the_one_pass_form(tmp_path):
    """bf16 table storage through the speculative one-pass tail with the clip ACTIVE (TLSAN_LAZY_ONE_PASS=3: by default only
    HBM-resident bf16 tables take this form, tlsan_api_plan.hip `plan_tail`).  The rows are written with coefficient 1
    (stochastic rounding at the magnitude of w - lr g), corrected by k_spec_commit (a second rounding) and read back through
    the folded table scale (a third): a stored element may be off by one bf16 ulp of the SPECULATIVE value plus two of the
    result -- not more; fp32 parameters keep the usual bound; two runs are bitwise equal.  (The split form, the default for
    cache-resident bf16 tables, rounds once: test_bf16_tables.)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = make_config(U=40, I=60, C=9, d=128, max_gradient_norm=0.02, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=41))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=48, Sn=4, seed=42)
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.7, clip=0.02)
    _, spec, _ = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.7, clip=1e30)      # what coefficient 1 writes first
    assert info["coef"] < 0.1
    outs = []
    for rep in range(2):
        f = str(tmp_path / ("run%d.npz" % rep))
        r = subprocess.run([sys.executable, "-c", _BF16_CLIP_DUMP % root, f], cwd=root, env=dict(os.environ, TLSAN_LAZY_ONE_PASS="3"),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(dict(np.load(f)))
    assert abs(float(outs[0]["loss"]) - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(float(outs[0]["gnorm"]) - info["norm"]) < 3e-4 * info["norm"]
    ulp_of = lambda x: 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 1e-30))) - 7)
    worst = 0.0
    for k in newp:
        assert np.array_equal(outs[0][k], outs[1][k]), k
        a, r = np.asarray(outs[0][k], np.float64).reshape(p[k].shape), newp[k]
        if k in BF16_TABLES:
            bound = ulp_of(spec[k]) + 2.0 * ulp_of(np.maximum(np.abs(r), np.abs(a)))
            assert (np.abs(a - r) <= bound * 1.001).all(), (k, float((np.abs(a - r) / bound).max()))
            worst = max(worst, float((np.abs(a - r) / ulp_of(r)).max()))
        else:
            du, dr = a - p[k], r - p[k]
            assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 2e-7, k
    assert worst > 3.0      # (the case does exercise the second rounding: otherwise it checks nothing the split form's test does not)


# (shape of the model, Model keywords, first batch size): the products a prefetched index may carry, each on the smallest
# shape that reaches it -- the rules are those of the planning unit, tlsan_amd/csrc/tlsan_api_plan.hip
_PREFETCH_CASES = {
    # d = 128 with 8 heads and at most 64 groups of 16 takes 8-sample groups (`train_group`, TLSAN_NW4 = 1): no ranking;
    # B <= 32 C: no category list; C < TLSAN_CSEG_MIN_CATES = 2048: no category segments
    "groups_of_8": (dict(d=128), dict(l2_mode="lazy"), 40),
    # `balanced`: 16 < B <= BAL_CAP, Sn > 0, at most FUSED_DK_MAX_GROUPS = 256 groups, I <= 2^18, and d = 64 has no small
    # group -- the index writes a ranking and the step reads it
    "ranking": (dict(d=64, Ls=10), dict(l2_mode="lazy"), 40),
    # Ls = 33 > TLSAN_LS_MAX = 10: streamed windows, ranked by window length (by_window = 1)
    "ranking_by_window": (dict(d=64, Ls=33), dict(l2_mode="lazy"), 40),
    # `uc_by_list`: B = 72 .. 86 > 32 C = 64 (and <= UC_LIST_CAP): k_uc_fill leaves the samples of every category
    "category_list": (dict(d=128, C=2), dict(l2_mode="lazy"), 72),
    # `cate_seg`: C = 2100 >= TLSAN_CSEG_MIN_CATES = 2048 and no category list (B <= 32 C)
    "category_segments": (dict(d=128, I=2300, C=2100), dict(l2_mode="lazy"), 40),
    # dense L2 sweeps every row: the index is built without TLSAN_INDEX_FOR_LAZY_SGD (offsets of every row)
    "full_index": (dict(d=128), dict(l2_mode="dense"), 40),
    # the index is planned without hyper-parameters, i.e. for the 8-sample groups of "groups_of_8"; with dropout the step
    # runs 16-sample groups (`train_group`: the small-group kernel is built without dropout) -- neither may touch a
    # ranking.  The keep / drop pattern is Model.dropout_seed(step): the same in all four runs.
    "dropout": (dict(d=128, dropout=0.2), dict(l2_mode="lazy"), 40),
}


@pytest.mark.parametrize("case", list(_PREFETCH_CASES))
def test_prefetched_index_equals_inline(case):
    """train_async(next_batch=..., after_next=...) builds the destination index of the next batch(es) on a second
    stream (tlsan_batch_index) one or two steps ahead; the result must be bitwise the same as building it inside the
    step, for batches of different shapes -- and for every optional product of the index (_PREFETCH_CASES: a ranking
    of the batch in either form, the category list, category segments, the full index of a dense-L2 step), which the
    prefetching call plans from the dims and the batch alone and the step reads one or two steps later."""
    shape, kw, B0 = _PREFETCH_CASES[case]
    cfg = make_config(**dict(dict(U=60, I=80, C=9, regulation_rate=1e-3), **shape))
    p = p32(random_params(cfg, seed=31))
    _, cat = random_batch(cfg, B=8, Sn=2, seed=0)
    batches = [batch_tuple(random_batch(cfg, B=B0 + 7 * (s % 3), Sn=1 + s % 4, seed=300 + s)[0]) for s in range(7)]
    runs = []
    for prefetch in (0, 1, 2, 3):     # none / one step ahead / two steps ahead / two ahead, announced irregularly
        m = model(cfg, cat, p, **kw)
        dbs = [m.device_batch(b) for b in batches]
        for s, db in enumerate(dbs):
            nxt = dbs[s + 1] if (prefetch and s + 1 < len(dbs)) else None
            nn = dbs[s + 2] if (prefetch >= 2 and s + 2 < len(dbs) and (prefetch == 2 or s % 2 == 0)) else None
            m.train_async(db, 0.6, next_batch=nxt, after_next=nn)
        runs.append(m.get_params())
    for r in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(runs[0][k], r[k]), k
    # announcing a batch and then training another one is an error (its uses are already counted)
    m = model(cfg, cat, p, **kw)
    dbs = [m.device_batch(b) for b in batches[:3]]
    m.train_async(dbs[0], 0.6, next_batch=dbs[1])
    with pytest.raises(RuntimeError):
        m.train_async(dbs[2], 0.6)


def test_full_scale_properties():
    """BASELINE.json configs[2] at full size (U=39991, I=22048, C=673, d=128, batch 4096): size-independent properties of
    the train step over three steps (one step at this size against the oracle itself: tests/test_gpu_configs.py,
    test_c3_electronics_one_step_matches_oracle).
      * determinism: two runs of 3 steps are bitwise equal;
      * the lazy-L2 step is the reference's dense-L2 step: after folding the scale, parameters of
        l2_mode=lazy and l2_mode=dense agree to fp32 rounding, losses and norms too;
      * untouched rows are not written in lazy mode;
      * checksums: the item_b gradient sums to the sum of d loss/d logit, and equals minus the
        change of item_b divided by the step; the per-use square sum of the step output is the
        sum of squares of every per-use row (recomputed from tlsan_grads with reg = 0 is not
        possible at this size, so it is pinned through the clip norm: gnorm^2 = sq_rows +
        reg^2 * ||tables||^2 + ||dense grads||^2)."""
    from tlsan_amd import synth
    cfg = synth.make_config("electronics")
    icl = synth.item_cate_list(cfg)
    batches = synth.make_batches(cfg, 3, 4096, seed=77)
    runs = {}
    for mode in ("lazy", "lazy", "dense"):
        m = model(cfg, icl, l2_mode=mode)
        p0 = m.get_params()
        before_user = m.user_emb.clone()
        losses, norms = [], []
        for b in batches:
            losses.append(m.train(None, b, 1.0))
            norms.append(m.last_gnorm())
        if mode == "lazy":   # (before get_params: reading the parameters folds the scale into the tables)
            touched = np.zeros(cfg["user_count"], bool)
            for b in batches:
                touched[np.asarray(b[0])] = True
            same = (m.user_emb == before_user).all(dim=1).cpu().numpy()
            assert same[~touched].all() and not same[touched].any()
        out = dict(params=m.get_params(), losses=losses, norms=norms)
        key = mode if mode not in runs else mode + "2"
        runs[key] = out
    for k in runs["lazy"]["params"]:
        assert np.array_equal(runs["lazy"]["params"][k], runs["lazy2"]["params"][k]), k
    assert runs["lazy"]["losses"] == runs["lazy2"]["losses"]
    assert np.allclose(runs["lazy"]["losses"], runs["dense"]["losses"], rtol=2e-6, atol=0)
    assert np.allclose(runs["lazy"]["norms"], runs["dense"]["norms"], rtol=1e-5, atol=0)
    for k in runs["lazy"]["params"]:
        a, d_ = np.asarray(runs["lazy"]["params"][k], np.float64), np.asarray(runs["dense"]["params"][k], np.float64)
        assert np.abs(a - d_).max() <= 2e-6 * np.abs(d_).max() + 1e-9, k
    # checksum of the step: item_b moves by -step * (sum of the per-use bias gradients) and its
    # total change is -step * sum_b dl_b, where sum_b dl_b = mean(sigmoid(logit) - y)
    m = model(cfg, icl, l2_mode="lazy")
    b = batches[0]
    db = m.device_batch(b)
    li, _, _, _ = m.forward(b, is_test=False)
    logit = li.cpu().numpy().astype(np.float64)
    y = np.asarray(b[2], np.float64)
    dl_sum = ((1.0 / (1.0 + np.exp(-logit))) - y).sum() / len(y)
    ib0 = m.get_params()["item_b"].astype(np.float64)
    m.train(None, b, 1.0)
    coef = min(1.0, cfg["max_gradient_norm"] / m.last_gnorm())
    ib1 = m.get_params()["item_b"].astype(np.float64)
    assert abs((ib0 - ib1).sum() - coef * dl_sum) < 1e-5 * max(1.0, abs(dl_sum)) + 1e-7


@pytest.mark.parametrize("matrix_dtype", ["f32", "bf16"])
def test_full_scale_bf16(matrix_dtype):
    """BASELINE.json configs[2] in the precision it names -- bf16 table storage (and, second case, bf16 matrix
    operands) -- at its own size (U=39991, I=22048, C=673, d=128, batch 4096); properties over three steps (one step
    with bf16 tables against the oracle at this size: test_c3_electronics_one_step_matches_oracle):
      * determinism: two runs of 3 steps leave bitwise equal tables and losses (stochastic rounding included);
      * the L2 term and the clip norm follow the STORED values: the loss a step reports equals the BCE of its logits
        plus reg/2 * ||P * stored tables||^2 recomputed from the tables themselves, after three updates whose changes
        of the sum of squares were only ever accumulated incrementally;
      * lazy L2 is dense L2 within the stochastic-rounding bound: every element within a few bf16 ulps, no bias;
      * untouched rows are not written in lazy mode."""
    import torch
    from tlsan_amd import synth
    cfg = synth.make_config("electronics")
    icl = synth.item_cate_list(cfg)
    batches = synth.make_batches(cfg, 4, 4096, seed=78)
    reg = cfg["regulation_rate"]
    runs = {}
    for mode in ("lazy", "lazy", "dense"):
        m = model(cfg, icl, l2_mode=mode, table_dtype="bf16", matrix_dtype=matrix_dtype)
        assert m.item_emb.dtype == torch.bfloat16
        before_user = m.user_emb.clone()
        losses = [m.train(None, b, 1.0) for b in batches[:3]]
        assert all(np.isfinite(losses))
        if mode == "lazy":
            touched = np.zeros(cfg["user_count"], bool)
            for b in batches[:3]:
                touched[np.asarray(b[0])] = True
            same = (m.user_emb == before_user).all(dim=1).cpu().numpy()
            assert same[~touched].all()
            # bookkeeping of the stored values: BCE of the next batch's logits + the L2 term from the tables as stored
            b = batches[3]
            li, _, _, _ = m.forward(b, is_test=False)
            x = li.double().cpu().numpy()
            y = np.asarray(b[2], np.float64)
            bce = (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean()
            P = m.table_scale()
            sq = sum(float((t.double() * P).pow(2).sum().item()) for t in (m.item_emb, m.user_emb, m.cate_emb, m.usert_emb))
            want = bce + reg * 0.5 * sq
            got = m.train(None, b, 1.0)
            assert abs(got - want) < 2e-5 * max(1.0, abs(want)), (got, want)
            losses.append(got)
        runs[mode if mode not in runs else mode + "2"] = dict(params=m.get_params(), losses=losses)
    for k in runs["lazy"]["params"]:
        assert np.array_equal(runs["lazy"]["params"][k], runs["lazy2"]["params"][k]), k
    assert runs["lazy"]["losses"] == runs["lazy2"]["losses"]
    assert np.allclose(runs["lazy"]["losses"][:3], runs["dense"]["losses"], rtol=2e-3, atol=0)
    # (the lazy run took one step more than the dense one above: compare fresh runs of three steps each)
    pl = model(cfg, icl, l2_mode="lazy", table_dtype="bf16", matrix_dtype=matrix_dtype)
    pd = model(cfg, icl, l2_mode="dense", table_dtype="bf16", matrix_dtype=matrix_dtype)
    for b in batches[:3]:
        pl.train_async(b, 1.0)
        pd.train_async(b, 1.0)
    ql, qd = pl.get_params(), pd.get_params()
    for k in ("item_emb", "user_emb", "cate_emb"):
        a, d_ = np.asarray(ql[k], np.float64), np.asarray(qd[k], np.float64)
        # (ulp of the element, not below the ulp of 0.01: an element that crosses zero has no meaningful own ulp)
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(d_), 0.01))) - 7)
        # dense: every element rounded once per step; lazy: touched rows once per step, the scale folded in at the read
        # (two trajectories whose roundings differ also see slightly different gradients: a tail of a few more ulps)
        dev = np.abs(a - d_) / ulp
        assert (dev <= 6.0).mean() > 0.999 and dev.max() <= 24.0, (k, dev.max(), (dev <= 6.0).mean())
        assert abs(((a - d_) / ulp).mean()) < 0.05, k
    for k in ("usert_emb", "item_b", "gamma"):
        a, d_ = np.asarray(ql[k], np.float64), np.asarray(qd[k], np.float64)
        assert np.abs(a - d_).max() <= 2e-3 * np.abs(d_).max() + 1e-6, k


def test_periodic_scale_fold_in_long_lazy_runs():
    """lazy L2 folds the table scale into the tables on a fixed schedule (Model.renorm_every) so that
    P never underflows; folding must not change what is trained."""
    cfg = make_config(U=40, I=60, C=9, d=64, regulation_rate=2e-2)
    p = p32(random_params(cfg, seed=71))
    _, cat = random_batch(cfg, B=8, Sn=2, seed=0)
    batches = [random_batch(cfg, B=30, Sn=3, seed=700 + s)[0] for s in range(7)]
    q = dict(p)
    for b in batches:
        _, q, _ = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=1.0)
    for every in (0, 3):
        m = model(cfg, cat, p, l2_mode="lazy")
        m.renorm_every = every
        for b in batches:
            m.train_async(batch_tuple(b), 1.0)
        if every:
            assert m.table_scale() > 0.97     # folded at step 6, one step since
        else:
            assert m.table_scale() < 0.9      # 7 steps of (1 - lr c reg)
        got = m.get_params()
        for k in q:
            g = np.asarray(got[k], np.float64).reshape(q[k].shape)
            assert np.abs(g - q[k]).max() < 5e-4 * np.abs(q[k]).max() + 1e-6, (every, k)


@pytest.mark.parametrize("l2_mode", ["dense", "lazy"])
def test_bf16_tables(l2_mode):
    """table_dtype='bf16' (BASELINE.json configs[2] names bf16 tables; a build extension, the reference
    is fp32): item_emb / user_emb / cate_emb are stored as bfloat16, arithmetic stays fp32.
      * forward and gradients equal the fp64 oracle evaluated on the stored (rounded) parameters;
      * after a step every bf16 element is one of the two bf16 neighbours of the exact update
        (stochastic rounding), the fp32 parameters match the oracle as usual;
      * the rounding is unbiased on average and deterministic (same bits on a second run);
      * the L2 / clip-norm bookkeeping follows the STORED values (loss of the next step matches the
        oracle evaluated on the stored parameters)."""
    cfg = make_config(U=60, I=90, C=9, d=128, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=81))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=64, Sn=4, seed=82)
    b2, _ = random_batch(cfg, B=64, Sn=3, seed=83)
    m = model(cfg, cat, p, l2_mode=l2_mode, table_dtype="bf16")
    got0 = m.get_params()
    for k in p:
        assert np.array_equal(np.asarray(got0[k], np.float64).reshape(p[k].shape), p[k]), k   # stored exactly
    # forward + gradients on the stored parameters
    out = orc.forward(p, cat, b, 8)
    li, _, _, _ = m.forward(batch_tuple(b), is_test=False)
    assert np.abs(li.cpu().numpy() - out["logits"]).max() < 1e-4
    g = m.grads(batch_tuple(b))
    _, _, ref_g, _ = orc.backward(p, cat, b, 8, cfg["regulation_rate"])
    for k in ref_g:
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.abs(a - r).max() < 2e-4 * np.abs(r).max() + 1e-6, k
    # one step: stochastic rounding lands on a bf16 neighbour of the exact update
    loss, q, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.7)
    runs = []
    for rep in range(2):
        mm = model(cfg, cat, p, l2_mode=l2_mode, table_dtype="bf16")
        l = mm.train(None, batch_tuple(b), 0.7)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
        l2 = mm.train(None, batch_tuple(b2), 0.7)           # second step: its loss carries the L2 term of the STORED tables
        runs.append((mm.get_params(), l2))
        if rep == 0:
            m1 = model(cfg, cat, p, l2_mode=l2_mode, table_dtype="bf16")
            m1.train(None, batch_tuple(b), 0.7)
            stored = {k: np.asarray(v, np.float64) for k, v in m1.get_params().items()}
            for k in q:
                a, r = stored[k].reshape(q[k].shape), q[k]
                if k in BF16_TABLES:
                    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
                    # (lazy: reading the parameters folds the table scale in, a second stochastic rounding)
                    nround = 2 if l2_mode == "lazy" else 1
                    assert (np.abs(a - r) <= ulp * (nround + 1e-3) + 1e-12).all(), k
                    assert np.array_equal(a.astype(np.float32), bf16_round(a)), k        # representable in bf16
                    bias = ((a - r) / ulp).mean()
                    assert abs(bias) < 0.06, (k, bias)                                    # unbiased: E[stored] = exact
                else:
                    du, dr = a - p[k], r - p[k]
                    assert np.abs(du - dr).max() < 2e-4 * (np.abs(dr).max() + 1e-9) + 2e-7, k
            ref_l2 = orc.train_step(stored, cat, b2, 8, cfg["regulation_rate"], lr=0.7)[0]
            assert abs(l2 - ref_l2) < 1e-4 * max(1.0, abs(ref_l2))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert runs[0][1] == runs[1][1]


@pytest.mark.parametrize("d,table_dtype,Ls", [(64, "f32", 10), (128, "f32", 10), (128, "bf16", 10), (256, "bf16", 10),
                                              (128, "f32", 20), (128, "bf16", 90), (64, "bf16", 33)])
def test_bf16_matrix_products(d, table_dtype, Ls):
    """matrix_dtype='bf16' (a build extension for BASELINE.json configs[2], which names bf16): the operands of
    every matrix product of the fused kernel are rounded to bfloat16, products and sums stay fp32.  NOT the
    north-star tolerance: with 8 significant bits per operand the logits agree with the fp64 oracle (on the
    stored parameters) to 1.5e-3 of their scale (1e-4 absolute with fp32 products), every gradient to 15 % of its
    L2 norm (b2 of both blocks excepted: mathematically zero), the loss to 5e-4.  Stated here so that the
    tolerance is part of the interface; the arithmetic is still deterministic (bitwise equal on a second run),
    and training at the reference's protocol reaches the same AUC (scripts/readme_band.py --matrix_dtype bf16)."""
    cfg = make_config(U=300, I=400, C=17, d=d, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=7))
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=96, Sn=4, seed=8)
    ref = orc.forward(p, cat, b, 8)
    loss, _, ref_g, _ = orc.backward(p, cat, b, 8, cfg["regulation_rate"])
    scale = np.abs(ref["logits"]).max()          # (Ls > 10: the streamed-window kernels)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, table_dtype=table_dtype, matrix_dtype="bf16")
        g = m.grads(batch_tuple(b))
        outs.append(g)
    g = outs[0]
    err = np.abs(g["logits"] - ref["logits"]).max()
    assert 1e-5 < err < 1.5e-3 * scale + 1e-3, (err, scale)      # (and really bf16: far above the fp32 path's 1e-6)
    assert abs(g["loss"] - loss) < 5e-4 * max(1.0, abs(loss))
    for k in ref_g:
        if k.endswith("_b2"):
            continue
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.linalg.norm(a - r) < 0.15 * np.linalg.norm(r) + 1e-9, (k, np.linalg.norm(a - r) / np.linalg.norm(r))
    for k in outs[0]["grads"]:
        assert np.array_equal(outs[0]["grads"][k], outs[1]["grads"][k]), k
    # a train step: lazy == dense to fp32 rounding in this mode too
    ms = [model(cfg, cat, p, l2_mode=l2, table_dtype=table_dtype, matrix_dtype="bf16") for l2 in ("dense", "lazy")]
    ls = [m.train(None, batch_tuple(b), 0.5) for m in ms]
    assert abs(ls[0] - ls[1]) < 1e-5 * max(1.0, abs(ls[0]))
    pa, pb = ms[0].get_params(), ms[1].get_params()
    for k in pa:
        tol = 2e-6 if table_dtype == "f32" else 2e-2     # (bf16 tables: two stochastic roundings apart)
        assert np.abs(np.asarray(pa[k], np.float64) - pb[k]).max() <= tol * np.abs(pa[k]).max() + 1e-9, k


@pytest.mark.parametrize("d,table_dtype,rate,Ls", [(64, "f32", 0.2, 10), (128, "bf16", 0.3, 10), (128, "f32", 0.3, 33),
                                                  (256, "f32", 0.4, 10)])
def test_dropout_with_bf16_matrix_products(d, table_dtype, rate, Ls):
    """config['dropout'] > 0 (model.py:116-118, 428-431) with matrix_dtype='bf16' (round 5; refused before): the
    same keep / drop pattern as the fp32 kernels draw -- a train step follows the oracle's step under that pattern
    to the bf16 tolerances of test_bf16_matrix_products (loss 5e-4, parameter changes to 15 % of their norm), far
    inside the distance to the step WITHOUT the pattern; a second model repeats it bitwise."""
    cfg = make_config(U=60, I=80, C=9, d=d, regulation_rate=1e-3, dropout=rate, Ls=Ls)
    p = p32(random_params(cfg, seed=97))
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=45, Sn=3, seed=98)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, table_dtype=table_dtype, matrix_dtype="bf16")
        seed = m.dropout_seed()
        l = m.train(None, batch_tuple(b), 0.6)
        outs.append((l, m.get_params()))
    loss, newq, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.6, dropout=(rate, seed))
    plain = orc.loss_fn(p, cat, b, 8, cfg["regulation_rate"])
    l, got = outs[0]
    tol = 5e-4 * max(1.0, abs(loss))
    assert abs(l - loss) < tol, (l, loss, plain)
    assert abs(plain - loss) > 4 * tol, (plain, loss)          # the pattern matters, well beyond the bf16 tolerance
    for k in ("fwa1_W1", "fwa1_W2", "fwa2_W1", "fwa2_W2", "dense_K", "dense_b"):
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = newq[k] - p[k]
        assert np.linalg.norm(du - dr) < 0.15 * np.linalg.norm(dr) + 1e-9, (k, np.linalg.norm(du - dr) / np.linalg.norm(dr))
    if table_dtype == "f32":
        assert outs[0][0] == outs[1][0]
        for k in got:
            assert np.array_equal(np.asarray(got[k]), np.asarray(outs[1][1][k])), k


@pytest.mark.parametrize("optimizer,lr", [("adam", 0.05), ("rmsprop", 0.02), ("adadelta", 1.0)])
def test_other_optimizers_track_oracle(optimizer, lr, tmp_path):
    """model.py:188-193: adam | rmsprop | adadelta with TF 1.8's defaults, every row of the regularised
    tables updated every step, clipped gradients; parameters AND both accumulators follow the oracle.
    The step counter / accumulators survive save + restore."""
    cfg = make_config(U=30, I=45, C=7, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer=optimizer,
                      model_dir=str(tmp_path))
    p = p32(random_params(cfg, seed=61))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=36, Sn=1 + s % 3, seed=600 + s)[0] for s in range(5)]
    m = model(cfg, cat, p)
    q, st = dict(p), orc.init_opt_state(p, optimizer)
    for n, b in enumerate(batches):
        prev = q
        loss, q, info = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=lr, clip=0.05, optimizer=optimizer,
                                       opt_state=st)
        assert info["coef"] < 1.0                 # the clip is active
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        got = m.get_params()
        for k in q:
            if k.endswith("_b2"):
                # the softmax over positions is invariant to b2, so its gradient is rounding noise (1e-14 in
                # fp64, 1e-9 in fp32) which Adam normalises to +-lr: not comparable, and without effect
                continue
            step = np.abs(q[k] - prev[k]).max()
            assert np.abs(np.asarray(got[k], np.float64).reshape(q[k].shape) - q[k]).max() < 2e-3 * step * (n + 1) + 1e-7, (n, k)
        if n == 2:                                # checkpoint round trip in the middle of the run
            path = m.save()
            m = model(cfg, cat, None)
            m.restore(None, path)
    s1, s2 = m.get_slots()
    for k in q:
        if k.endswith("_b2"):
            continue
        for got, ref in ((s1[k], st["slot1"][k]), (s2[k], st["slot2"][k])):
            assert np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max() < 2e-3 * np.abs(ref).max() + 1e-9, k
    assert np.array_equal(m.dense_KT.cpu().numpy(), m.get_params()["dense_K"].T)
    with pytest.raises(NotImplementedError):
        model(cfg, cat, p, l2_mode="lazy")


@pytest.mark.parametrize("l2_mode", ["lazy", "dense"])
def test_large_tables_take_the_two_level_scan(l2_mode):
    """Tables of more than 16 chunks of 4096 rows build their destination index with per-chunk sums
    (k_scan_block_sums + k_index_scan) instead of the single launch; the step must not notice.
    Two steps on 300k users / 150k items against the oracle."""
    cfg = make_config(U=300_000, I=150_000, C=40, d=64, regulation_rate=1e-3, max_gradient_norm=5.0)
    p = p32(random_params(cfg, seed=81))
    _, cat = random_batch(cfg, B=4, Sn=2, seed=0)
    batches = [random_batch(cfg, B=48, Sn=2 + s, seed=810 + s)[0] for s in range(2)]
    m = model(cfg, cat, p, l2_mode=l2_mode)
    q = dict(p)
    for b in batches:
        loss, newq, info = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=0.9)
        l = m.train(None, batch_tuple(b), 0.9)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
        assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
        q = newq
    got = m.get_params()
    for k in q:
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = q[k] - p[k]
        assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 3e-7, k


@pytest.mark.parametrize("d,rate,Ls", [(64, 0.2, 10), (128, 0.35, 10), (256, 0.5, 10), (128, 0.3, 33), (64, 0.25, 90)])
def test_dropout_training_matches_oracle(d, rate, Ls):
    """config['dropout'] > 0 (model.py:116-118, 428-431): tf.nn.dropout on the inputs of the two maps of
    both attention blocks, train steps only.  With the same keep / drop pattern (a hash of seed, sample,
    block, position, map, channel) three train steps follow the oracle; evaluation does not drop."""
    cfg = make_config(U=40, I=60, C=9, d=d, regulation_rate=1e-3, dropout=rate, Ls=Ls)   # (Ls > 10: streamed window)
    p = p32(random_params(cfg, seed=91))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=37, Sn=2 + s, seed=910 + s)[0] for s in range(3)]
    m = model(cfg, cat, p)
    q = dict(p)
    for n, b in enumerate(batches):
        seed = m.dropout_seed()
        loss, newq, info = orc.train_step(q, cat, b, 8, cfg["regulation_rate"], lr=0.6, dropout=(rate, seed))
        plain = orc.loss_fn(q, cat, b, 8, cfg["regulation_rate"])
        assert abs(plain - loss) > 1e-5                        # the pattern matters
        l = m.train(None, batch_tuple(b), 0.6)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss)), (n, l, loss, plain)
        assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
        got = m.get_params()
        for k in newq:
            du = np.asarray(got[k], np.float64).reshape(q[k].shape) - q[k]
            dr = newq[k] - q[k]
            assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 3e-7, (n, k)
        q = {k: np.asarray(got[k], np.float64).reshape(newq[k].shape) for k in newq}   # follow the device
    # forward / evaluation: no dropout
    li, _, _, _ = m.forward(batch_tuple(batches[0]), is_test=False)
    ref = orc.forward(q, cat, batches[0], 8)["logits"]
    assert np.abs(li.cpu().numpy() - ref).max() < LOGIT_TOL


@pytest.mark.parametrize("d,Ls", [(64, 10), (128, 10), (128, 24), (64, 40)])
def test_empty_histories(d, Ls):
    """sl = 0 (no long-term history; the reference's placeholders allow it although build_dataset.py never
    emits it): every position is masked, exp_mask leaves -1e30 everywhere (model.py:384, 480-483), the
    softmax is uniform over rows that are all zero -> the long summary is exactly 0 and nothing flows back
    into the window.  Mixed with ordinary samples, forward and one train step against the oracle."""
    cfg = make_config(U=30, I=50, C=7, d=d, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=95))
    b, cat = random_batch(cfg, B=41, Sn=3, seed=96)
    b["sl"][::3] = 0
    if Ls > 10:
        b["sl"][16:32] = 0          # (streamed windows: a whole workgroup pass without a single window entry)
    ar = np.arange(cfg["Ls"])[None, :]
    b["hist_i"] = np.where(ar < b["sl"][:, None], b["hist_i"], 0)
    b["hist_t"] = np.where(ar < b["sl"][:, None], b["hist_t"], 0).astype(np.float32)
    ref = orc.forward(p, cat, b, 8)
    m = model(cfg, cat, p)
    li, _, _, _ = m.forward(batch_tuple(b), is_test=False)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.5)
    l = m.train(None, batch_tuple(b), 0.5)
    assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
    got = m.get_params()
    for k in newp:
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 3e-7, k


@pytest.mark.parametrize("l2_mode,C,clip", [("lazy", 4, 5.0), ("dense", 4, 5.0), ("lazy", 40, 5.0), ("lazy", 40, 0.02), ("lazy", 4, 0.02)])
def test_one_hot_row_takes_every_use(l2_mode, C, clip):
    """Collisions at their worst: every sample is the same user, every window and session the same item,
    the candidate the last item of the table -- one destination row receives all 3000+ per-use gradient
    rows (long segments finished by the whole wavefront, one category with every use), one user row
    all 256; one train step against the oracle, bitwise reproducible.  Four categories: a category shared by several
    row-sum workgroups (summed beside the one-pass update of the item / user rows, updated by the commit launch); forty:
    the one-pass form throughout, whose hot-row workgroup updates the row itself -- with coefficient 1, and corrected by
    k_spec_commit when the step is clipped (clip 0.02)."""
    cfg = make_config(U=9, I=31, C=C, d=128, regulation_rate=1e-3, max_gradient_norm=clip)
    p = p32(random_params(cfg, seed=97))
    b, cat = random_batch(cfg, B=256, Sn=2, seed=98, full=True)
    b["u"][:] = cfg["user_count"] - 1
    b["hist_i"][:] = 7
    b["hist_i_new"][:] = 7
    b["i"][:] = cfg["item_count"] - 1
    b["u_cate"][:] = int(cat[7])
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.5, clip=clip)
    assert (info["coef"] < 1.0) == (clip < 1.0)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, l2_mode=l2_mode)
        l = m.train(None, batch_tuple(b), 0.5)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
        assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
        outs.append(m.get_params())
    for k in newp:
        assert np.array_equal(outs[0][k], outs[1][k]), k
        du = np.asarray(outs[0][k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 3e-7, k


@pytest.mark.parametrize("extra", [["--optimizer", "adam", "--learning_rate", "0.01"],
                                   ["--dropout", "0.2"],
                                   ["--l2_mode", "lazy", "--table_dtype", "bf16"]])
def test_train_driver_variants(extra, tmp_path):
    """The driver's other switches on the real Clothing tuples: 200 steps with adam, with dropout, and
    with lazy L2 + bf16 tables run through, learn (loss falls) and leave a restorable checkpoint."""
    import os
    from tlsan_amd import train as T
    from tlsan_amd.model import Model
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    args = T.parse(["--dataset", ds, "--max_steps", "200", "--eval_freq", "100", "--quiet", "--eval_topk", "0",
                    "--model_dir", str(tmp_path / "ck")] + extra)
    res = T.train(args)
    assert res["steps"] == 200 and np.isfinite(res["final_auc"]) and 0.8 < res["final_auc"] < 1.0
    files = sorted(os.listdir(tmp_path / "ck"))
    assert "TLSAN-200.npz" in files and "TLSAN-200.json" in files
    z = np.load(tmp_path / "ck" / "TLSAN-200.npz")
    assert int(z["global_step"]) == 200 and all(np.isfinite(z[k]).all() for k in ("item_emb", "user_emb", "dense_K"))
    if "adam" in extra:
        assert "slot1/item_emb" in z.files and "slot2/dense_K" in z.files


def test_user_index_from_a_sort_of_the_batch():
    """Tables of 65 536 users or more take the user side of a batch's destination index from a partitioned counting sort of
    the batch's user ids (IsortArgs: three short launches whose blocks keep a bucket's counters in the LDS) instead of
    counters and a scan over the table.  TLSAN_ISORT_MIN=1 (read once per process) sends every table that way: the oracle
    tests of train steps -- small user tables, so batches full of repeated users -- must hold."""
    import subprocess, sys
    env = dict(os.environ, TLSAN_ISORT_MIN="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-k",
                        "test_train_step_matches_oracle or test_multi_step_tracks_oracle_and_is_deterministic or test_lazy_l2_matches_dense_oracle "
                        "or test_full_size_batch_matches_oracle or test_long_windows_streamed or test_graph_replay_equals_eager or test_prefetched_index_equals_inline"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    mt = re.search(r"(\d+) passed", r.stdout)      # (the selection is by name: it must not shrink silently)
    assert mt and int(mt.group(1)) >= 18, r.stdout[-2000:]


_ISORT_DIGEST = r'''
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from tests.helpers import make_config, random_batch, random_params
from tlsan_amd.model import Model
h = hashlib.sha256()
for d, Ls, I, C in ((128, 10, 70000, 2100), (64, 33, 9000, 300), (128, 10, 300, 40)):
    cfg = make_config(U=500, I=I, C=C, d=d, Ls=Ls, regulation_rate=1e-3)
    p = {k: np.asarray(v, np.float32) for k, v in random_params(cfg, seed=11).items()}
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    m = Model(cfg, cat, l2_mode="lazy")
    m.set_params(p)
    bs = [random_batch(cfg, B=700, Sn=1 + s, seed=40 + s)[0] for s in range(4)]
    for b in bs[:2]:                 # (collisions: ids folded onto a few hundred rows, some of them hot)
        for k in ("hist_i", "hist_i_new", "i"):
            b[k] %%= 257
    tup = lambda b: (b["u"], b["i"], b["y"], b["hist_i"], b["hist_i_new"], b["hist_t"], b["sl"], b["sl_new"], b["u_cate"])
    dbs = [m.device_batch(tup(b)) for b in bs]
    for s in range(len(dbs)):        # (announced one / two ahead: the index of the batches after this one is built on the side stream)
        m.train_async(dbs[s], 0.7, next_batch=dbs[s + 1] if s + 1 < len(dbs) else None, after_next=dbs[s + 2] if s + 2 < len(dbs) else None)
    h.update(np.float32(m._out[0].item()).tobytes())
    got = m.get_params()
    for k in sorted(got):
        h.update(np.ascontiguousarray(got[k]).tobytes())
print("DIGEST", h.hexdigest())
'''


def test_item_index_from_a_counting_sort_of_the_batch():
    """The item-side twin of the test above.  Item tables of 65 536 rows or more, in a lazy-L2 SGD step with category
    segments, take the item side of a batch's destination index from a partitioned counting sort of the batch's item ids
    (IsortArgs: buckets of consecutive ids, a bucket's counters in the LDS) instead of a global counter per table row
    and two scans over them.  TLSAN_ISORT_MIN=1 with TLSAN_CSEG_MIN=1 (both read once per process) sends every table
    that way: the oracle tests of lazy train steps must hold, and -- first positions are assigned in id order either
    way -- four steps on three table shapes must leave the SAME BITS as the counter path (losses and every parameter)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TLSAN_ISORT_MIN="1", TLSAN_CSEG_MIN="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-k",
                        "test_lazy_l2_matches_dense_oracle or test_lazy_is_deterministic or test_category_segments_match_oracle "
                        "or test_full_size_batch_matches_oracle or test_long_windows_streamed or test_one_hot_row_takes_every_use "
                        "or test_prefetched_index_equals_inline or test_periodic_scale_fold"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) >= 18, r.stdout[-2000:]
    digests = []
    for isort_min in ("1", str(1 << 30)):
        env = dict(os.environ, TLSAN_ISORT_MIN=isort_min, TLSAN_CSEG_MIN="1")
        r = subprocess.run([sys.executable, "-c", _ISORT_DIGEST % root], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        digests.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1])
    assert digests[0] == digests[1], digests


_RANK_DUMP = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tests.helpers import make_config, random_batch, random_params
from tlsan_amd.model import Model
cfg = make_config(U=300, I=500, C=23, d=128, regulation_rate=1e-3)
p = {k: np.asarray(v, np.float32) for k, v in random_params(cfg, seed=5).items()}
_, cat = random_batch(cfg, B=8, Sn=3, seed=0)
m = Model(cfg, cat, l2_mode="lazy")
m.set_params(p)
tup = lambda b: (b["u"], b["i"], b["y"], b["hist_i"], b["hist_i_new"], b["hist_t"], b["sl"], b["sl_new"], b["u_cate"])
losses = [m.train(None, tup(random_batch(cfg, B=1224, Sn=2 + s, seed=70 + s)[0]), 0.5) for s in range(3)]   # (1224 = 76 groups of 16 + 8: a partial last group; > 1024: 16-sample workgroups)
np.savez(sys.argv[1], losses=np.asarray(losses), **m.get_params())
'''


def test_ranking_of_the_batch_changes_results_by_rounding_only(tmp_path):
    """which samples share a workgroup of the fused kernel is a ranked function of the batch where that was measured
    to win (tlsan_api_plan.hip `balanced`: table size, group count, TLSAN_BAL_REG) -- so the fp32 grouping of the per-group partial
    sums, and with it the last bits of a step, depend on those.  Each setting is bitwise reproducible by itself (the
    determinism tests); across settings results may differ by fp32 rounding ONLY: three lazy steps of a batch with a partial
    last group, ranked (TLSAN_BAL_REG=1) and in the batch's own order (=0)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for reg in ("1", "0"):
        f = str(tmp_path / ("bal%s.npz" % reg))
        r = subprocess.run([sys.executable, "-c", _RANK_DUMP % root, f], cwd=root, env=dict(os.environ, TLSAN_BAL_REG=reg),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out.append(dict(np.load(f)))
    a, b = out
    assert np.allclose(a["losses"], b["losses"], rtol=2e-6, atol=0)
    differ = False
    for k in a:
        if k == "losses":
            continue
        scale = float(np.abs(a[k]).max()) + 1e-12
        assert np.abs(a[k].astype(np.float64) - b[k]).max() <= 2e-5 * scale, k
        differ = differ or not np.array_equal(a[k], b[k])
    assert differ      # (the ranking did change the grouping: otherwise this test checks nothing)


@pytest.mark.parametrize("d,di,Ls", [(128, 96, 10), (128, 32, 10), (64, 48, 10), (64, 16, 10), (128, 96, 24), (256, 128, 10)])
def test_unequal_embedding_widths(d, di, Ls):
    """The reference's `itemid_embedding_size` and `cateid_embedding_size` are separate flags (train.py:26-49; only their sum
    must equal hidden_units, model.py:100-109): item / user rows of `di` floats beside category rows of `d - di`.  Every
    other test takes the two halves equal.  Forward logits and one train step (lazy and dense L2) against the oracle with
    the concatenated row split anywhere a 16-byte piece allows (rows wider than 64 floats take the wide row workgroups)."""
    cfg = make_config(U=60, I=80, C=9, d=d, Ls=Ls, di=di, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=d + di))
    b, cat = random_batch(cfg, B=45, Sn=4, seed=di)
    ref = orc.forward(p, cat, b, 8)
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.7)
    for l2 in ("lazy", "dense"):
        m = model(cfg, cat, p, l2_mode=l2)
        li, _, ut, _ = m.forward(batch_tuple(b), is_test=False, want_u_t=True)
        assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL, l2
        assert np.abs(ut.cpu().numpy() - ref["u_t"]).max() < LOGIT_TOL, l2
        got_loss = m.train(None, batch_tuple(b), 0.7)
        assert abs(got_loss - loss) < 1e-4 * max(1.0, abs(loss)), l2
        assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"], l2
        got = m.get_params()
        for k in newp:
            du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
            dr = newp[k] - p[k]
            assert np.abs(du - dr).max() < 2e-4 * (np.abs(dr).max() + 1e-9) + 2e-7, (l2, k)


_CSPL_DIGEST = r'''
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from tests.helpers import make_config, random_batch, random_params
from tlsan_amd.model import Model
h = hashlib.sha256()
# (categories of 300-450 items: shared by item; of 60-70: by use position -- category_split, tlsan_api_plan.hip)
for d, Ls, C, td, I in ((128, 10, 3, "f32", 900), (128, 90, 2, "f32", 900), (64, 33, 5, "f32", 300), (128, 70, 3, "bf16", 200)):
    cfg = make_config(U=500, I=I, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=1e4)
    p = {k: np.asarray(v, np.float32) for k, v in random_params(cfg, seed=13).items()}
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    m = Model(cfg, cat, l2_mode="lazy", table_dtype=td)
    m.set_params(p)
    bs = [random_batch(cfg, B=700, Sn=1 + s, seed=60 + s)[0] for s in range(4)]
    for b in bs[:2]:                 # (collisions: some rows hot)
        for k in ("hist_i", "hist_i_new", "i"):
            b[k] %%= 61
    tup = lambda b: (b["u"], b["i"], b["y"], b["hist_i"], b["hist_i_new"], b["hist_t"], b["sl"], b["sl_new"], b["u_cate"])
    dbs = [m.device_batch(tup(b)) for b in bs]
    for s in range(len(dbs)):
        m.train_async(dbs[s], 0.7, next_batch=dbs[s + 1] if s + 1 < len(dbs) else None, after_next=dbs[s + 2] if s + 2 < len(dbs) else None)
    h.update(np.float32(m._out[0].item()).tobytes())
    m.fold_scale()
    got = m.get_params()
    for k in sorted(got):
        h.update(np.ascontiguousarray(got[k]).tobytes())
print("DIGEST", h.hexdigest())
'''


@pytest.mark.parametrize("d,Ls,C,clip", [(128, 10, 3, 5.0), (128, 10, 3, 0.02), (128, 90, 2, 5.0), (128, 90, 2, 0.05), (64, 33, 5, 0.02),
                                         (128, 10, 8, 5.0)])
def test_shared_categories_in_the_one_pass_form(d, Ls, C, clip):
    """Few, large categories (Movies-TV: 15) are shared by several row-sum workgroups that add exact doubles into Rc64
    (category_split) -- a sum no single workgroup holds, so their rows cannot be updated in the pass that sums them.  The
    lazy-L2 step then takes the one-pass update for the item and user rows only (k_finalize_update<.., CSPL>: the category
    workgroups sum beside them) and updates the category rows in the commit launch, which knows the coefficient
    (k_spec_commit<.., CSPL>).  One train step against the oracle, clip inactive and active, user rows of up to 128 floats
    and wider (d = 128 with a 90-entry window: two passes of the narrow form), categories of 100-250 items (shared by
    item) and of 62 (C = 8: shared by use position), bitwise reproducible."""
    cfg = make_config(U=300, I=500, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=clip)
    p = p32(random_params(cfg, seed=131))
    b, cat = random_batch(cfg, B=640, Sn=3, seed=132)
    for k in ("hist_i", "hist_i_new"):     # (some hot rows)
        b[k][::3] %= 5
    assert 640 * (Ls + 3 + 2) // C > 512       # (category_split: more than one workgroup per category)
    loss, newp, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=0.5, clip=clip)
    assert (info["coef"] < 1.0) == (clip < 1.0)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, l2_mode="lazy")
        l = m.train(None, batch_tuple(b), 0.5)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
        assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
        outs.append(m.get_params())
    for k in newp:
        assert np.array_equal(outs[0][k], outs[1][k]), k
        du = np.asarray(outs[0][k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < 3e-4 * (np.abs(dr).max() + 1e-9) + 3e-7, k


def test_shared_categories_one_pass_equals_the_split_form():
    """Unclipped steps of the form above leave the SAME BITS as the split form (row sums beside the finalize, then
    k_update_lazy; TLSAN_LAZY_ONE_PASS=0, read once per process): four steps announced two ahead on four table shapes, fp32 and
    bf16 tables (TLSAN_LAZY_ONE_PASS=3 sends cache-resident bf16 tables through the one-pass form too), losses and every
    parameter -- and as the same form with fewer workgroups per category (TLSAN_CSPLIT_FINE=0)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    # (third run: round 5's rule for how many workgroups share a category -- 27 instead of 64 here; the sums are exact, so
    #  the number of workgroups that share a category must not change a bit either)
    # (fourth run: the sharers deal a category's uses out by item instead of by position)
    for one_pass, fine, pos in (("3", "1", "1"), ("0", "1", "1"), ("3", "0", "1"), ("3", "1", "0")):
        env = dict(os.environ, TLSAN_LAZY_ONE_PASS=one_pass, TLSAN_CSPLIT_FINE=fine, TLSAN_CSPLIT_POS=pos)
        r = subprocess.run([sys.executable, "-c", _CSPL_DIGEST % root], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        digests.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1])
    assert len(set(digests)) == 1, digests


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_lazy_sum_of_squares_tracks_the_tables(d, table_dtype):
    """Lazy L2 keeps the stored tables' sum of squares (StateHdr::St, state bytes 32..40) from per-workgroup records of its
    changes, which the next step folds in (DeltaRec, tlsan_state.h): after any sequence of updates it equals the tables'
    own.  Batches of varying B and Sn make the records an update leaves shrink and grow; a large L2 rate at lr = 1 makes
    one workgroup's change a visible part of the sum; the first steps clip (the correcting pass adds to its records); the
    scale is folded into the tables every third step.  The tables are large enough that fp32 rounding in that fold stays far
    below the tolerance.  A second run that takes gradients after every step (a fold without an update) ends bit-equal."""
    import torch
    clip = {64: 13.5, 128: 17.0}[d]     # (above the norm of the later steps, below that of the first: profiled with the oracle)
    cfg = make_config(U=3000, I=4000, C=40, d=d, regulation_rate=0.05, max_gradient_norm=clip)
    p = p32(random_params(cfg, seed=1301))
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = bf16_round(p[k]).astype(np.float64)
    _, cat = random_batch(cfg, B=8, Sn=2, seed=1300)
    shapes = [(64, 1), (5, 3), (40, 5), (1, 2), (64, 4), (17, 1)]
    batches = [batch_tuple(random_batch(cfg, B=B, Sn=Sn, seed=1310 + k)[0]) for k, (B, Sn) in enumerate(shapes)]
    probe = batch_tuple(random_batch(cfg, B=9, Sn=2, seed=1320)[0])
    runs = []
    for every_step in (False, True):
        m = model(cfg, cat, p, l2_mode="lazy", table_dtype=table_dtype)
        m.renorm_every = 3
        losses, gnorms = [], []
        for b in batches:
            losses.append(m.train(None, b, 1.0))
            gnorms.append(m.last_gnorm())
            if every_step:
                m.grads(probe)
        m.grads(probe)                     # (folds the last step's records)
        St = float(m.state[32:40].view(torch.float64).item())
        ref = sum(float(getattr(m, k).double().pow(2).sum().item()) for k in orc.REG_TABLES)
        assert abs(St - ref) <= 1e-9 * ref, (St, ref)
        assert gnorms[0] > clip and min(gnorms) < clip, gnorms
        runs.append((St, losses, m.get_params()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1], (runs[0][:2], runs[1][:2])
    for k in runs[0][2]:
        assert np.array_equal(runs[0][2][k], runs[1][2][k]), k


def test_speculative_one_pass_lazy_update():
    """Tables that live in HBM (more than 512 MB of user / item rows, category segments) take the lazy-L2 step as ONE pass
    over the used rows BESIDE the finalize, with clip coefficient 1, and a second launch that commits the table scale and --
    after a clipped step only -- corrects the rows (k_finalize_update, tlsan_finalize_rows.h / k_spec_commit, tlsan_spec_commit.h).
    TLSAN_LAZY_ONE_PASS=2 with TLSAN_CSEG_MIN=1 (both read once per process) sends every table that way: the oracle tests of
    lazy train steps must hold -- clip inactive AND active (test_lazy_l2_matches_dense_oracle[0.02]: the correcting pass),
    bf16 tables, hipGraph replay, a diverged step -- and unclipped steps must leave the SAME BITS as the split form (row sums
    beside the finalize, then k_update_lazy; TLSAN_LAZY_ONE_PASS=0)."""
    import re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sel = ("test_lazy_l2_matches_dense_oracle or test_lazy_is_deterministic or test_category_segments_match_oracle "
           "or test_full_size_batch_matches_oracle or test_one_hot_row_takes_every_use or test_multi_step_tracks_oracle "
           "or test_prefetched_index_equals_inline or test_periodic_scale_fold or test_bf16_tables or test_graph_replay_equals_eager "
           "or test_nonfinite_inputs_give_nonfinite_loss or test_real_fixture_batches or test_lazy_sum_of_squares")
    # (3: every table shape the one-pass form takes -- the item-walk category workgroups and the hot-row workgroups of
    #  tables with few categories, which TLSAN_CSEG_MIN=1 would hide)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-k", sel],
                       cwd=root, env=dict(os.environ, TLSAN_LAZY_ONE_PASS="3"), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) >= 25, r.stdout[-2000:]
    # (TLSAN_SPEC_ITEM_BLOCKS=3: the launch carries three item-row workgroups, each walking every third block of 16 used rows
    #  -- the form tables of millions of rows take, whose batches can touch far more rows than they do)
    env = dict(os.environ, TLSAN_LAZY_ONE_PASS="2", TLSAN_CSEG_MIN="1", TLSAN_SPEC_ITEM_BLOCKS="3")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-k",
                        "test_lazy_l2_matches_dense_oracle or test_lazy_is_deterministic or test_category_segments_match_oracle "
                        "or test_full_size_batch_matches_oracle or test_one_hot_row_takes_every_use or test_multi_step_tracks_oracle "
                        "or test_prefetched_index_equals_inline or test_periodic_scale_fold or test_bf16_tables or test_graph_replay_equals_eager "
                        "or test_nonfinite_inputs_give_nonfinite_loss or test_real_fixture_batches or test_lazy_sum_of_squares"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) >= 25, r.stdout[-2000:]
    # (the split form: the row sums beside the finalize, then k_update_lazy)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-k", "test_lazy_sum_of_squares"],
                       cwd=root, env=dict(os.environ, TLSAN_LAZY_ONE_PASS="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) == 4, r.stdout[-2000:]
    digests = []
    for one_pass in ("2", "0"):
        env = dict(os.environ, TLSAN_LAZY_ONE_PASS=one_pass, TLSAN_CSEG_MIN="1")
        r = subprocess.run([sys.executable, "-c", _ISORT_DIGEST % root], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        digests.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1])
    assert digests[0] == digests[1], digests


@pytest.mark.parametrize("d,Ls", [(128, 10), (64, 10), (128, 33), (256, 10)])
def test_dropout_with_bf16_tables(d, Ls):
    """config['dropout'] > 0 with table_dtype='bf16' (round 3 refused the combination): the gradients equal the oracle's
    at the stored (bf16-rounded) tables under the same keep / drop pattern, and a training step is reproducible."""
    rate = 0.3
    cfg = make_config(U=40, I=60, C=9, d=d, regulation_rate=1e-3, dropout=rate, Ls=Ls)
    p = p32(random_params(cfg, seed=95))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=37, Sn=3, seed=951)
    m = model(cfg, cat, p, l2_mode="lazy", table_dtype="bf16")
    seed = m.dropout_seed()
    g = m.grads(batch_tuple(b))
    loss, _, ref_g, _ = orc.backward(p, cat, b, 8, cfg["regulation_rate"], dropout=(rate, seed))
    plain = orc.loss_fn(p, cat, b, 8, cfg["regulation_rate"])
    assert abs(plain - loss) > 1e-5                        # the pattern matters
    assert abs(g["loss"] - loss) < 1e-4 * max(1.0, abs(loss))
    for k in ref_g:
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.abs(a - r).max() < 3e-4 * np.abs(r).max() + 1e-6, k
    outs = []
    for rep in range(2):
        mm = model(cfg, cat, p, l2_mode="lazy", table_dtype="bf16")
        mm.train(None, batch_tuple(b), 0.6)
        outs.append(mm.get_params())
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("d,Ls,B,Sn", [(128, 10, 37, 4), (64, 10, 50, 0), (256, 10, 21, 3), (128, 33, 40, 2), (64, 90, 19, 5), (256, 20, 18, 1)])
def test_attention_weights_match_oracle(d, Ls, B, Sn):
    """The reference keeps the two attention-weight tensors on the model (model.py:122: self.att0, self.att1 = `soft` of
    feature_wise_attention, :386-394, heads split along the batch axis).  Model.forward(want_att=True) leaves them as
    [H*B, Ls, d/H] and [H*B, 1+Sn, d/H], row h*B + b -- windows in registers and streamed, sessions of every length
    including none, exactly 0 on masked positions."""
    cfg = make_config(U=50, I=80, C=8, d=d, Ls=Ls)
    p = p32(random_params(cfg, seed=d + Ls))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=Ls + B, test=True)
    b["sl"][:3] = [Ls, 1, max(1, Ls - 1)]
    m = model(cfg, cat, p)
    li, lj, _, _ = m.forward(batch_tuple(b, test=True), is_test=True, want_att=True)
    ref = orc.forward(p, cat, dict(b, y=np.zeros(B)), 8)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    H = 8
    for got, want, T, length in ((m.att0, ref["att0"], Ls, b["sl"]), (m.att1, ref["att1"], Sn + 1, b["sl_new"] + 1)):
        w = np.asarray(want).transpose(2, 0, 1, 3).reshape(H * B, T, d // H)      # [B, T, H, dh] -> row h*B + b
        g = got.cpu().numpy()
        assert g.shape == w.shape
        assert np.abs(g - w).max() < 2e-5, np.abs(g - w).max()
        masked = np.arange(T)[None, :] >= np.tile(np.asarray(length), H)[:, None]  # [H*B, T]
        assert (g[masked] == 0.0).all()                                            # masked positions: exactly 0
        assert np.abs(g.sum(1) - 1.0).max() < 1e-5                                 # a softmax over positions per channel


@pytest.mark.parametrize("optimizer,lr", [("adam", 0.01), ("rmsprop", 0.01), ("adadelta", 1.0)])
def test_other_optimizers_with_bf16_tables(optimizer, lr):
    """adam / rmsprop / adadelta on bf16 tables (round 3 refused the combination): the accumulators stay fp32 and follow
    the oracle run from the stored (bf16-rounded) tables; every stored table element is one of the two bf16 neighbours of
    the oracle's updated value (stochastic rounding on the write-back); the fp32-kept parameters match as usual; two runs
    leave the same bits."""
    cfg = make_config(U=30, I=45, C=7, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer=optimizer)
    p = p32(random_params(cfg, seed=63))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=36, Sn=3, seed=631)
    st = orc.init_opt_state(p, optimizer)
    loss, q, info = orc.train_step(p, cat, b, 8, cfg["regulation_rate"], lr=lr, clip=0.05, optimizer=optimizer, opt_state=st)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, table_dtype="bf16")
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        outs.append((m.get_params(), m.get_slots()))
    got, (s1, s2) = outs[0]
    for k in q:
        assert np.array_equal(outs[0][0][k], outs[1][0][k]), k
        if k.endswith("_b2"):
            continue              # (gradient = rounding noise, see test_other_optimizers_track_oracle)
        a, r = np.asarray(got[k], np.float64).reshape(q[k].shape), q[k]
        if k in BF16_TABLES:
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
            assert (np.abs(a - r) <= ulp * 1.001 + 2e-3 * np.abs(r - p[k]).max()).all(), k
            assert np.array_equal(a.astype(np.float32), bf16_round(a)), k
        else:
            step = np.abs(r - p[k]).max()
            assert np.abs(a - r).max() < 2e-3 * step + 1e-7, k
        for gs, ref in ((s1[k], st["slot1"][k]), (s2[k], st["slot2"][k])):
            assert np.abs(np.asarray(gs, np.float64).reshape(ref.shape) - ref).max() < 2e-3 * np.abs(ref).max() + 1e-9, k


@pytest.mark.parametrize("nw4", ["0", "2"])
def test_d128_parity_in_both_workgroup_geometries(nw4):
    """d = 128 training launches of up to 1024 sequences take the 8-sample geometry (Geo<128, 16, 4>) by default, so the
    small-batch parity tests above only reach the 16-sample kernel -- the one the bench shape runs -- through the B = 4096
    cases.  TLSAN_NW4 (read once per process) pins the geometry: 0 = 16-sample workgroups always, 2 = 8-sample always.
    The d = 128 gradient / train-step / bf16 / category-segment cases must hold to the oracle in both."""
    import subprocess, sys
    env = dict(os.environ, TLSAN_NW4=nw4)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_parity.py", "-m", "gpu", "-q", "-x", "-k",
                        "(test_gradients and 128) or test_train_step_matches_oracle or test_multi_step_tracks_oracle_and_is_deterministic "
                        "or (test_category_segments_match_oracle and 128-10) or test_bf16_tables or (test_bf16_matrix_products and 128) "
                        "or test_lazy_l2_matches_dense_oracle or test_long_sessions_and_short_window or (test_empty_histories and 128-10)"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    # (the selection is by NAME -- a renamed or re-parametrised case must not silently shrink it)
    import re
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) >= 23, r.stdout[-2000:]


@pytest.mark.parametrize("mm", ["f32", "bf16"])
@pytest.mark.parametrize("d,Ls", [(64, 10), (128, 10), (256, 33)])
def test_nonfinite_inputs_give_nonfinite_loss(d, Ls, mm):
    """A diverged run must look diverged (TLSAN/model.py:171: the reference's loss goes NaN, printed at train.py:205).
    The d <= 128 units and the streamed d = 256 unit are built with -fno-honor-nans / -fno-signed-zeros
    (tlsan_amd/build.py): the compiler may assume no NaN reaches a comparison or fmaxf.  Plant a NaN and a +Inf in a
    gathered item_emb row, a gathered user_emb row and a dense weight (fwa1_W2: every score of the long block), one at a
    time, and require a non-finite loss AND global norm from the train step, lazy and dense L2; after a step with a NaN
    norm the clip coefficient (clip_coef, tlsan_common.h) has handed it on to the parameters, as TF's clip_by_global_norm does."""
    cfg = make_config(U=30, I=50, C=7, d=d, Ls=Ls)
    p0 = p32(random_params(cfg, seed=5 * d + Ls))
    b, cat = random_batch(cfg, B=40, Sn=3, seed=d + 1)
    it, us = int(b["hist_i"][0, 0]), int(b["u"][3])          # (sl >= 1: position 0 is a valid window entry)
    for key, idx in (("item_emb", (it, 5)), ("user_emb", (us, 2)), ("fwa1_W2", (1, 2))):
        for bad in (np.nan, np.inf):
            for l2 in ("lazy", "dense"):
                p = {k: v.copy() for k, v in p0.items()}
                p[key][idx] = bad
                m = model(cfg, cat, p, l2_mode=l2, matrix_dtype=mm)
                loss = m.train(None, batch_tuple(b), 1.0)
                assert not np.isfinite(loss), (key, bad, l2, loss)
                assert not np.isfinite(m.last_gnorm()), (key, bad, l2, m.last_gnorm())
                if np.isnan(m.last_gnorm()):   # (a NaN norm poisons every clipped gradient, as TF's min(1 / norm, 1 / clip) does;
                    got = m.get_params()       #  a +Inf norm clips to coefficient 0: finite gradients then move nothing)
                    assert not np.isfinite(got["dense_K"]).all(), (key, bad, l2)
    # ... and a healthy step stays finite (the check is not vacuous)
    m = model(cfg, cat, p0, l2_mode="lazy", matrix_dtype=mm)
    assert np.isfinite(m.train(None, batch_tuple(b), 1.0)) and np.isfinite(m.last_gnorm())


"""GPU tests of the (hidden_units, num_heads) pairs beside the 8-head ones: 64/4 (16 channels per head), 128/16 (8, two
heads per 16-channel block) and 128/4 (32, two 16-channel blocks per column at d = 128).  Every feature of the fused
kernel against the oracle with the same number of heads, at the tolerances of tests/test_gpu_parity.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.helpers import BF16_TABLES, batch_tuple, bf16_round, make_config, model, p32, random_batch, random_params
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-4
PAIRS = [(64, 4), (128, 16), (128, 4)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_update(got, p, newp, tol, floor, what=""):
    for k in newp:
        du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
        dr = newp[k] - p[k]
        assert np.abs(du - dr).max() < tol * (np.abs(dr).max() + 1e-9) + floor, (what, k)


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("B,Sn", [(1, 0), (37, 3), (300, 18)])
def test_forward_logits(d, H, B, Sn):
    cfg = make_config(U=70, I=90, C=11, d=d, H=H)
    p = p32(random_params(cfg, seed=d + H + B))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=B + Sn, test=True)
    m = model(cfg, cat, p)
    li, lj, ut, _ = m.forward(batch_tuple(b, True), is_test=True, want_u_t=True)
    ref = orc.forward(p, cat, b, H)
    bn = dict(b); bn["i"] = b["j"]
    refj = orc.forward(p, cat, bn, H)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    assert np.abs(lj.cpu().numpy() - refj["logits"]).max() < LOGIT_TOL
    assert np.abs(ut.cpu().numpy() - ref["u_t"]).max() < LOGIT_TOL
    auc = m.eval_auc(None, batch_tuple(b, True))
    assert auc == pytest.approx(float(np.mean(ref["logits"] - refj["logits"] > 0)), abs=1e-6)


@pytest.mark.parametrize("d,H", PAIRS)
def test_gradients_both_norm_modes(d, H):
    cfg = make_config(U=30, I=50, C=7, d=d, H=H)
    p = p32(random_params(cfg, seed=3 * d + H))
    b, cat = random_batch(cfg, B=45, Sn=4, seed=d * 7 + H)
    reg = cfg["regulation_rate"]
    loss, logits, g, sparse = orc.backward(p, cat, b, H, reg)
    m = model(cfg, cat, p)
    out = m.grads(batch_tuple(b))
    assert np.abs(out["logits"] - logits).max() < LOGIT_TOL
    assert abs(out["loss"] - loss) < 1e-4 * max(1.0, abs(loss))
    for k in g:
        gk = np.asarray(out["grads"][k], np.float64).reshape(g[k].shape)
        err = np.abs(gk - g[k]).max()
        assert err < 2e-4 * np.abs(g[k]).max() + 1e-6, (k, err, np.abs(g[k]).max())
    n18 = orc.global_norm(p, g, sparse, reg, "tf18")
    assert abs(out["gnorm"] - n18) < 2e-4 * n18
    out2 = model(cfg, cat, p, norm_mode="dedup").grads(batch_tuple(b))
    nd = orc.global_norm(p, g, sparse, reg, "dedup")
    assert abs(out2["gnorm"] - nd) < 2e-4 * nd


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("l2_mode", ["dense", "lazy"])
@pytest.mark.parametrize("clip", [5.0, 0.02])
def test_train_step_matches_oracle(d, H, l2_mode, clip):
    cfg = make_config(U=40, I=60, C=9, d=d, H=H, max_gradient_norm=clip, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=11 + H))
    b, cat = random_batch(cfg, B=48, Sn=4, seed=12)
    loss, newp, info = orc.train_step(p, cat, b, H, cfg["regulation_rate"], lr=0.7, clip=clip)
    assert (info["coef"] < 1.0) == (clip < 1)
    m = model(cfg, cat, p, l2_mode=l2_mode)
    l = m.train(None, batch_tuple(b), 0.7)
    assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
    assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
    got = m.get_params()
    _check_update(got, p, newp, 2e-4, 2e-7)
    assert np.array_equal(m.dense_KT.cpu().numpy(), got["dense_K"].T)


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("l2_mode", ["dense", "lazy"])
def test_three_steps_track_oracle_and_are_bitwise_reproducible(d, H, l2_mode):
    cfg = make_config(U=25, I=35, C=5, d=d, H=H, regulation_rate=5e-5)
    p = p32(random_params(cfg, seed=21 + H))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=40, Sn=1 + s, seed=100 + s)[0] for s in range(3)]
    runs = []
    for rep in range(2):
        m = model(cfg, cat, p, l2_mode=l2_mode)
        losses = [m.train(None, batch_tuple(b), 0.5) for b in batches]
        runs.append((losses, m.get_params()))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
    q = dict(p)
    ref = []
    for b in batches:
        l, q, _ = orc.train_step(q, cat, b, H, cfg["regulation_rate"], lr=0.5)
        ref.append(l)
    assert np.allclose(runs[0][0], ref, rtol=2e-4, atol=1e-5)
    for k in q:
        got = np.asarray(runs[0][1][k], np.float64).reshape(q[k].shape)
        assert np.abs(got - q[k]).max() < 5e-4 * np.abs(q[k]).max() + 1e-6, k


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("Ls,B,Sn", [(33, 50, 3), (90, 37, 5)])
def test_long_windows_streamed(d, H, Ls, B, Sn):
    cfg = make_config(U=50, I=150, C=8, d=d, H=H, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=Ls + d + H))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=Ls)
    b["sl"][:4] = [Ls, 1, Ls - 1, min(Ls, 11)]
    ar = np.arange(Ls)[None, :]
    b["hist_i"] = np.where(ar < b["sl"][:, None], np.random.RandomState(2).randint(0, 150, (B, Ls)), 0)
    b["hist_t"] = np.where(ar < b["sl"][:, None], (1.0 / np.random.RandomState(3).randint(1, 13, (B, Ls))), 0).astype(np.float32)
    ref = orc.forward(p, cat, b, H)
    tb = dict(b); tb["j"] = b["i"][::-1].copy()
    li, lj, ut, _ = model(cfg, cat, p).forward(batch_tuple(tb, True), is_test=True, want_u_t=True)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    assert np.abs(ut.cpu().numpy() - ref["u_t"]).max() < LOGIT_TOL
    loss, newp, info = orc.train_step(p, cat, b, H, cfg["regulation_rate"], lr=0.6)
    for l2 in ("dense", "lazy"):
        m = model(cfg, cat, p, l2_mode=l2)
        l = m.train(None, batch_tuple(b), 0.6)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), l2
        assert abs(m.last_gnorm() - info["norm"]) < 3e-4 * info["norm"], l2
        _check_update(m.get_params(), p, newp, 3e-4, 5e-7, l2)


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("Ls,Sn", [(10, 4), (33, 2)])
def test_attention_weights_match_oracle(d, H, Ls, Sn):
    B = 37
    cfg = make_config(U=50, I=80, C=8, d=d, H=H, Ls=Ls)
    p = p32(random_params(cfg, seed=d + Ls + H))
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=Ls + B, test=True)
    b["sl"][:3] = [Ls, 1, max(1, Ls - 1)]
    m = model(cfg, cat, p)
    li, _, _, _ = m.forward(batch_tuple(b, test=True), is_test=True, want_att=True)
    ref = orc.forward(p, cat, dict(b, y=np.zeros(B)), H)
    assert np.abs(li.cpu().numpy() - ref["logits"]).max() < LOGIT_TOL
    for got, want, T, length in ((m.att0, ref["att0"], Ls, b["sl"]), (m.att1, ref["att1"], Sn + 1, b["sl_new"] + 1)):
        w = np.asarray(want).transpose(2, 0, 1, 3).reshape(H * B, T, d // H)      # [B, T, H, dh] -> row h*B + b
        g = got.cpu().numpy()
        assert g.shape == w.shape
        assert np.abs(g - w).max() < 2e-5, np.abs(g - w).max()
        masked = np.arange(T)[None, :] >= np.tile(np.asarray(length), H)[:, None]
        assert (g[masked] == 0.0).all()
        assert np.abs(g.sum(1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("Ls", [10, 33])
def test_dropout_training_matches_oracle(d, H, Ls):
    rate = 0.3
    cfg = make_config(U=40, I=60, C=9, d=d, H=H, regulation_rate=1e-3, dropout=rate, Ls=Ls)
    p = p32(random_params(cfg, seed=91 + H))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=37, Sn=2 + s, seed=910 + s)[0] for s in range(2)]
    m = model(cfg, cat, p)
    q = dict(p)
    for n, b in enumerate(batches):
        seed = m.dropout_seed()
        loss, newq, info = orc.train_step(q, cat, b, H, cfg["regulation_rate"], lr=0.6, dropout=(rate, seed))
        plain = orc.loss_fn(q, cat, b, H, cfg["regulation_rate"])
        assert abs(plain - loss) > 1e-5
        l = m.train(None, batch_tuple(b), 0.6)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss)), (n, l, loss, plain)
        assert abs(m.last_gnorm() - info["norm"]) < 2e-4 * info["norm"]
        got = m.get_params()
        _check_update(got, q, newq, 3e-4, 3e-7, n)
        q = {k: np.asarray(got[k], np.float64).reshape(newq[k].shape) for k in newq}
    li, _, _, _ = m.forward(batch_tuple(batches[0]), is_test=False)
    assert np.abs(li.cpu().numpy() - orc.forward(q, cat, batches[0], H)["logits"]).max() < LOGIT_TOL


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("l2_mode,Ls", [("dense", 10), ("lazy", 10), ("lazy", 33)])
def test_bf16_tables(d, H, l2_mode, Ls):
    """bf16 tables: forward and gradients equal the oracle on the stored parameters; a step lands every table element on
    a bf16 neighbour of the exact update, the rest follows the oracle, and a second run repeats it bitwise."""
    cfg = make_config(U=60, I=90, C=9, d=d, H=H, Ls=Ls, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=81 + H))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=64, Sn=4, seed=82)
    m = model(cfg, cat, p, l2_mode=l2_mode, table_dtype="bf16")
    li, _, _, _ = m.forward(batch_tuple(b), is_test=False)
    assert np.abs(li.cpu().numpy() - orc.forward(p, cat, b, H)["logits"]).max() < 1e-4
    g = m.grads(batch_tuple(b))
    _, _, ref_g, _ = orc.backward(p, cat, b, H, cfg["regulation_rate"])
    for k in ref_g:
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.abs(a - r).max() < 2e-4 * np.abs(r).max() + 1e-6, k
    loss, q, info = orc.train_step(p, cat, b, H, cfg["regulation_rate"], lr=0.7)
    runs = []
    for rep in range(2):
        mm = model(cfg, cat, p, l2_mode=l2_mode, table_dtype="bf16")
        l = mm.train(None, batch_tuple(b), 0.7)
        assert abs(l - loss) < 1e-4 * max(1.0, abs(loss))
        runs.append(mm.get_params())
    for k in q:
        a, r = np.asarray(runs[0][k], np.float64).reshape(q[k].shape), q[k]
        if k in BF16_TABLES:
            # (the ulp of the larger of the two: lazy rounds twice, and a first rounding up to a power of two leaves the
            #  second one the next binade's ulp)
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(r), np.abs(a)), 1e-30))) - 7)
            nround = 2 if l2_mode == "lazy" else 1
            ratio = np.abs(a - r) / ulp
            w = np.unravel_index(np.argmax(ratio), ratio.shape)
            assert (np.abs(a - r) <= ulp * (nround + 1e-3) + 1e-12).all(), (k, ratio[w], a[w], r[w], p[k][w])
            assert np.array_equal(a.astype(np.float32), bf16_round(a)), k
        else:
            du, dr = a - p[k], r - p[k]
            assert np.abs(du - dr).max() < 2e-4 * (np.abs(dr).max() + 1e-9) + 2e-7, k
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("d,H", PAIRS)
@pytest.mark.parametrize("table_dtype,Ls,rate", [("f32", 10, 0.0), ("bf16", 33, 0.0), ("f32", 10, 0.3)])
def test_bf16_matrix_products(d, H, table_dtype, Ls, rate):
    """bf16 matrix operands, at test_bf16_matrix_products' tolerances (logits 1.5e-3 of their scale, gradients 15 % of
    their norm, loss 5e-4); with dropout, the step follows the oracle's under the same pattern to the same tolerances."""
    cfg = make_config(U=300, I=400, C=17, d=d, H=H, Ls=Ls, regulation_rate=1e-3, dropout=rate)
    p = p32(random_params(cfg, seed=7 + H))
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = bf16_round(p[k]).astype(np.float64)
    b, cat = random_batch(cfg, B=96, Sn=4, seed=8)
    if rate > 0:
        outs = []
        for rep in range(2):
            m = model(cfg, cat, p, table_dtype=table_dtype, matrix_dtype="bf16")
            seed = m.dropout_seed()
            outs.append((m.train(None, batch_tuple(b), 0.6), m.get_params()))
        loss, newq, _ = orc.train_step(p, cat, b, H, cfg["regulation_rate"], lr=0.6, dropout=(rate, seed))
        plain = orc.loss_fn(p, cat, b, H, cfg["regulation_rate"])
        l, got = outs[0]
        tol = 5e-4 * max(1.0, abs(loss))
        assert abs(l - loss) < tol and abs(plain - loss) > 4 * tol, (l, loss, plain)
        for k in ("fwa1_W1", "fwa1_W2", "fwa2_W1", "fwa2_W2", "dense_K", "dense_b"):
            du = np.asarray(got[k], np.float64).reshape(p[k].shape) - p[k]
            dr = newq[k] - p[k]
            assert np.linalg.norm(du - dr) < 0.15 * np.linalg.norm(dr) + 1e-9, k
        assert outs[0][0] == outs[1][0]
        return
    ref = orc.forward(p, cat, b, H)
    loss, _, ref_g, _ = orc.backward(p, cat, b, H, cfg["regulation_rate"])
    scale = np.abs(ref["logits"]).max()
    outs = [model(cfg, cat, p, table_dtype=table_dtype, matrix_dtype="bf16").grads(batch_tuple(b)) for _ in range(2)]
    g = outs[0]
    err = np.abs(g["logits"] - ref["logits"]).max()
    assert 1e-5 < err < 1.5e-3 * scale + 1e-3, (err, scale)
    assert abs(g["loss"] - loss) < 5e-4 * max(1.0, abs(loss))
    for k in ref_g:
        if k.endswith("_b2"):
            continue
        a, r = np.asarray(g["grads"][k], np.float64).reshape(ref_g[k].shape), ref_g[k]
        assert np.linalg.norm(a - r) < 0.15 * np.linalg.norm(r) + 1e-9, k
    for k in outs[0]["grads"]:
        assert np.array_equal(outs[0]["grads"][k], outs[1]["grads"][k]), k


@pytest.mark.parametrize("d,H", PAIRS)
def test_category_segments(d, H):
    """Tables of thousands of categories: the category half of the gradient rows goes to per-category segments (CSEG)."""
    cfg = make_config(U=70, I=2600, C=2100, d=d, H=H, Ls=10, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=91 + H))
    cat = np.random.RandomState(5).randint(0, 2100, 2600).astype(np.int32)
    b, _ = random_batch(cfg, B=41, Sn=3, seed=900)
    loss, newp, _ = orc.train_step(p, cat, b, H, cfg["regulation_rate"], lr=0.6)
    for l2 in ("dense", "lazy"):
        m = model(cfg, cat, p, l2_mode=l2)
        l = m.train(None, batch_tuple(b), 0.6)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), l2
        _check_update(m.get_params(), p, newp, 3e-4, 5e-7, l2)


@pytest.mark.parametrize("optimizer,lr", [("adam", 0.05), ("rmsprop", 0.02), ("adadelta", 1.0)])
@pytest.mark.parametrize("d,H", PAIRS)
def test_other_optimizers_and_checkpoints(d, H, optimizer, lr, tmp_path):
    cfg = make_config(U=30, I=45, C=7, d=d, H=H, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer=optimizer,
                      model_dir=str(tmp_path))
    p = p32(random_params(cfg, seed=61 + H))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=36, Sn=1 + s % 3, seed=600 + s)[0] for s in range(4)]
    m = model(cfg, cat, p)
    q, st = dict(p), orc.init_opt_state(p, optimizer)
    for n, b in enumerate(batches):
        prev = q
        loss, q, info = orc.train_step(q, cat, b, H, cfg["regulation_rate"], lr=lr, clip=0.05, optimizer=optimizer,
                                       opt_state=st)
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        got = m.get_params()
        for k in q:
            if k.endswith("_b2"):
                continue
            step = np.abs(q[k] - prev[k]).max()
            assert np.abs(np.asarray(got[k], np.float64).reshape(q[k].shape) - q[k]).max() < 2e-3 * step * (n + 1) + 1e-7, (n, k)
        if n == 1:
            path = m.save()
            m = model(cfg, cat, None)
            m.restore(None, path)


@pytest.mark.parametrize("d,H", PAIRS)
def test_save_restore_round_trip(d, H, tmp_path):
    cfg = make_config(U=30, I=45, C=7, d=d, H=H, regulation_rate=1e-3, model_dir=str(tmp_path))
    p = p32(random_params(cfg, seed=71 + H))
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    b1, _ = random_batch(cfg, B=36, Sn=2, seed=700)
    b2, _ = random_batch(cfg, B=36, Sn=3, seed=701)
    m = model(cfg, cat, p, l2_mode="lazy")
    m.train(None, batch_tuple(b1), 0.5)
    path = m.save()
    m2 = model(cfg, cat, None, l2_mode="lazy")
    m2.restore(None, path)
    a, c = m.get_params(), m2.get_params()
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    assert m.train(None, batch_tuple(b2), 0.5) == m2.train(None, batch_tuple(b2), 0.5)


@pytest.mark.parametrize("d,H", PAIRS)
def test_eval_ranks_and_metrics(d, H):
    cfg = make_config(U=60, I=333, C=13, d=d, H=H)
    p = p32(random_params(cfg, seed=31 + H))
    b, cat = random_batch(cfg, B=77, Sn=3, seed=32, test=True)
    m = model(cfg, cat, p)
    ranks = m.label_ranks(batch_tuple(b, True)).cpu().numpy()
    ref = orc.forward(p, cat, b, H)
    scores = orc.all_item_scores(p, cat, ref["u_t"])
    rr = orc.label_ranks(scores, b["i"])
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


def test_one_pass_lazy_tail_with_category_segments():
    """The speculative one-pass lazy update (k_finalize_update, with its correcting pass after a clipped step) and
    category segments at every new pair: the lazy tests above, in a child process with the switches of
    test_speculative_one_pass_lazy_update (read once per process)."""
    # (6 + 3 + 3 + 6 + 6 tests: every lazy step above, clipped ones with their correcting pass, bf16 tables included)
    sel = ("test_train_step_matches_oracle and lazy or test_three_steps_track and lazy or test_category_segments "
           "or test_long_windows_streamed or test_bf16_tables and lazy")
    env = dict(os.environ, TLSAN_LAZY_ONE_PASS="2", TLSAN_CSEG_MIN="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_heads.py", "-m", "gpu", "-q", "-x", "-k", sel],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) >= 24, r.stdout[-2000:]


def test_train_driver_with_four_heads(tmp_path):
    """tlsan_amd.train --num_heads 4 (d = 64: 16 channels per head) on the real Clothing tuples: AUC rises within 600 steps."""
    from tlsan_amd import train as T
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    res = T.train(T.parse(["--dataset", ds, "--max_steps", "600", "--eval_freq", "300", "--quiet", "--num_heads", "4",
                           "--model_dir", str(tmp_path / "ckpt")]))
    assert res["steps"] == 600
    assert res["final_auc"] > res["init_auc"] + 0.003
    assert len(res["prec"]) == 6 and 0.0 <= res["recall"][-1] <= 1.0


def _shard_worker(rank, world):
    from tlsan_amd.dist import ShardedModel
    d, H = 128, 4
    cfg = make_config(U=61, I=83, C=9, d=d, H=H, regulation_rate=1e-3)
    p = p32(random_params(cfg, seed=17))
    _, cat = random_batch(cfg, B=4, Sn=2, seed=0)
    steps = [[random_batch(cfg, B=24, Sn=3, seed=1000 + 10 * s + r)[0] for r in range(world)] for s in range(3)]
    m = ShardedModel(cfg, cat, device="cuda:0", l2_mode="lazy")
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    losses = []
    for per in steps:
        m.train_async(batch_tuple(per[rank]), 0.8)
        losses.append(float(m.last_loss.item()))
    got = m.gather_params()
    if rank == 0:
        q = dict(p)
        ref = []
        for per in steps:
            glob = {k: np.concatenate([b[k] for b in per], 0) for k in per[0]}
            l, q, _ = orc.train_step(q, cat, glob, H, cfg["regulation_rate"], lr=0.8)
            ref.append(l)
        assert np.allclose(losses, ref, rtol=2e-4, atol=1e-5), (losses, ref)
        for k in q:
            g = np.asarray(got[k], np.float64).reshape(q[k].shape)
            du, dr = g - p[k], q[k] - p[k]
            assert np.abs(du - dr).max() < 5e-4 * (np.abs(dr).max() + 1e-9) + 5e-7, k


def test_sharded_step_with_four_heads_at_d128():
    """The row-sharded step (tlsan_amd.dist) at 128/4: two processes sharing the GPU over gloo, three steps."""
    run_ranks(_shard_worker, 2)

"""Lazy Adam / RMSProp / Adadelta (TLSAN_OPT_LAZY) on the GPU against the restricted oracle: the dense optimizer's step
from the same parameters and slots (oracle.tlsan_oracle.train_step), after which every row the batch did not use is put
back, in W and both slots.  Used rows: users of b.u; items of the candidates and of the valid history / session positions;
categories of those items and of u_cate.  item_b: the candidates."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.helpers import BF16_TABLES, batch_tuple, bf16_round, make_config, model, p32, random_batch, random_params
from tests.lazy_opt_ref import (LR, ROW_TABLES, SPARSE_CATEGORY_CASES, check_step, compared, random_slots, restricted_step,
                                sync_amb, cover_all_batch)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop", "adadelta"])
def test_lazy_optimizers_track_the_restricted_oracle(optimizer, tmp_path):
    """Tables much larger than a batch with non-zero slots everywhere: five clipped steps and one unclipped one, a
    checkpoint round trip in the middle.  Loss, used rows and dense weights with their slots follow the restricted oracle;
    rows the step did not use keep W and both slots bit for bit."""
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=1e-3, max_gradient_norm=0.05,
                      optimizer="lazy_" + optimizer, model_dir=str(tmp_path))
    lr = LR[optimizer]
    p = p32(random_params(cfg, seed=71))
    st = random_slots(p, optimizer, 72)
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=16 + 4 * s, Sn=1 + s % 3, seed=700 + s)[0] for s in range(6)]
    m = model(cfg, cat, p, [st["slot1"], st["slot2"]])
    q = dict(p)
    for n, b in enumerate(batches):
        clip = 0.05 if n < 5 else 1e3
        m.config["max_gradient_norm"] = clip
        before = (m.get_params(), m.get_slots())
        prev = q
        loss, q, info, used = restricted_step(q, st, cat, b, cfg, lr, optimizer, clip)
        assert (info["coef"] < 1.0) == (n < 5)
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (n, l, loss)
        assert not used["user_emb"].all() and not used["item_emb"].all()
        check_step(m, q, st, prev, used, n + 1, exact_unused=before)
        sync_amb(m, q, st, used)
        if n == 2:                                # checkpoint round trip in the middle of the run
            path = m.save()
            m = model(cfg, cat, None)
            m.restore(None, path)
    assert m.table_scale() == 1.0


@pytest.mark.parametrize("optimizer,dropout,matrix_dtype", [("adam", 0.0, "f32"), ("rmsprop", 0.0, "f32"),
                                                          ("adadelta", 0.0, "f32"), ("adam", 0.2, "f32"),
                                                          ("rmsprop", 0.0, "bf16")])
def test_lazy_equals_dense_when_every_row_is_used(optimizer, dropout, matrix_dtype):
    """One batch that uses every row of every table: lazy_X and X from the same parameters and slots agree to fp32
    rounding, with dropout and bf16 matrix products as well (the same keep / drop pattern and products in both)."""
    cfg = make_config(U=40, I=60, C=7, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, dropout=dropout)
    lr = LR[optimizer]
    p = p32(random_params(cfg, seed=73))
    st = random_slots(p, optimizer, 74)
    _, cat = random_batch(cfg, B=8, Sn=3, seed=1)
    b = cover_all_batch(cfg, 740)
    out = []
    for name in (optimizer, "lazy_" + optimizer):
        m = model(dict(cfg, optimizer=name), cat, p, [st["slot1"], st["slot2"]], matrix_dtype=matrix_dtype)
        l = m.train(None, batch_tuple(b), lr)
        out.append((l, m.get_params(), m.get_slots()))
    (ld, pd, sd), (ll, pl, sl) = out
    assert abs(ld - ll) <= 1e-6 * max(1.0, abs(ld))
    for k in pd:
        scale = np.abs(pd[k] - np.asarray(p[k], np.float32)).max() + 1e-30
        assert np.abs(pl[k] - pd[k]).max() <= 1e-5 * scale + 1e-7, k
        for j in range(2):
            assert np.abs(sl[j][k] - sd[j][k]).max() <= 1e-5 * np.abs(sd[j][k]).max() + 1e-12, k


def _row_form_run(d, Ls, C, optimizer, B=24, Sn=3, steps=2, seed=80, U=200, I=300, clip=0.05, table_dtype="f32"):
    cfg = make_config(U=U, I=I, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=clip,
                      optimizer="lazy_" + optimizer)
    lr = LR[optimizer]
    p = p32(random_params(cfg, seed=seed))
    st = random_slots(p, optimizer, seed + 1)
    _, cat = random_batch(cfg, B=8, Sn=2, seed=seed + 2)
    m = model(cfg, cat, p, [st["slot1"], st["slot2"]], table_dtype=table_dtype)
    q = dict(p)
    for s in range(steps):
        b = random_batch(cfg, B=B, Sn=Sn, seed=seed + 10 + s)[0]
        before = (m.get_params(), m.get_slots())
        prev = q
        loss, q, info, used = restricted_step(q, st, cat, b, cfg, lr, optimizer, clip)
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (s, l, loss)
        check_step(m, q, st, prev, used, s + 1, exact_unused=before)
        sync_amb(m, q, st, used)


@pytest.mark.parametrize("d,Ls,C,optimizer", [(64, 10, 20, "adam"), (128, 10, 20, "rmsprop"), (256, 10, 20, "adadelta"),
                                              (128, 90, 20, "adam"), (64, 90, 12, "rmsprop"), (256, 90, 12, "adam"),
                                              (64, 10, 2, "adam"), (128, 10, 3, "adadelta")])
def test_lazy_row_forms(d, Ls, C, optimizer):
    """Narrow and wide rows (d = 64 / 128 / 256), streamed windows with wide user rows (Ls = 90), and few large
    categories that several row-sum workgroups share (the Rc64 sums the row update clears)."""
    B = 96 if C <= 3 else 24
    _row_form_run(d, Ls, C, optimizer, B=B)


def _sparse_category_run(optimizer, C, item_cates, ucate_cates, B, d=64, Ls=10, steps=2, seed=120):
    """A batch uses a small part of the category table: the items belong to `item_cates` only and u_cate names
    `ucate_cates` only, so some categories are reached only through items, some named only by u_cate, and the rest are
    unused -- those keep W and both slots bit for bit (check_step), the others follow the restricted oracle."""
    cfg = make_config(U=300, I=450, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=0.05,
                      optimizer="lazy_" + optimizer)
    lr = LR[optimizer]
    rng = np.random.RandomState(seed)
    cat = rng.choice(np.asarray(item_cates), cfg["item_count"]).astype(np.int32)
    p = p32(random_params(cfg, seed=seed + 1))
    st = random_slots(p, optimizer, seed + 2)
    m = model(cfg, cat, p, [st["slot1"], st["slot2"]])
    q = dict(p)
    only_items = only_ucate = unused = 0
    for s in range(steps):
        b = random_batch(cfg, B=B, Sn=3, seed=seed + 10 + s)[0]
        b["u_cate"] = rng.choice(np.asarray(ucate_cates), B).astype(np.int64)
        before = (m.get_params(), m.get_slots())
        prev = q
        loss, q, info, used = restricted_step(q, st, cat, b, cfg, lr, optimizer, 0.05)
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (s, l, loss)
        check_step(m, q, st, prev, used, s + 1, exact_unused=before)
        sync_amb(m, q, st, used)
        by_item = np.zeros(C, bool)
        by_item[cat[used["item_emb"]]] = True
        by_ucate = np.zeros(C, bool)
        by_ucate[b["u_cate"]] = True
        only_items += int((by_item & ~by_ucate).sum())
        only_ucate += int((by_ucate & ~by_item).sum())
        unused += int((~used["cate_emb"]).sum())
    assert only_items > 0 and only_ucate > 0 and unused > 0, (only_items, only_ucate, unused)


@pytest.mark.parametrize("optimizer,C,item_cates,ucate_cates,B,d", SPARSE_CATEGORY_CASES)
def test_lazy_leaves_unused_category_rows_alone(optimizer, C, item_cates, ucate_cates, B, d):
    _sparse_category_run(optimizer, C, item_cates, ucate_cates, B, d=d)


_CSEG = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_lazy_opt import _row_form_run
for opt in ("adam", "adadelta"):
    _row_form_run(64, 10, 40, opt, B=32, seed=90)
    _row_form_run(128, 24, 40, opt, B=32, seed=91)
from tests.lazy_opt_ref import SPARSE_CATEGORY_CASES
from tests.test_gpu_lazy_opt import _sparse_category_run
for optimizer, C, item_cates, ucate_cates, B, d in SPARSE_CATEGORY_CASES:
    _sparse_category_run(optimizer, C, item_cates, ucate_cates, B, d=d, seed=140)
print("ok")
"""


def test_lazy_with_category_segments():
    """Category segments (TLSAN_CSEG_MIN=1 in a child process: read once per process), the sparse category tables
    included: a category's segment then counts every use."""
    env = dict(os.environ, TLSAN_CSEG_MIN="1")
    r = subprocess.run([sys.executable, "-c", _CSEG, ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_lazy_step_on_a_scaled_state():
    """A C caller may run lazy-L2 SGD steps on the state first, so that the table scale P is not 1: the lazy optimizer's
    step then acts on the true values P * stored (as the forward pass and the loss do) and leaves P as it is."""
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=0.05, max_gradient_norm=0.05, optimizer="lazy_adam")
    p = p32(random_params(cfg, seed=131))
    st = random_slots(p, "adam", 132)
    _, cat = random_batch(cfg, B=8, Sn=3, seed=133)
    m = model(cfg, cat, p, [st["slot1"], st["slot2"]])
    copt, m._copt = m._copt, None            # two unclipped lazy-L2 SGD steps (tlsan_train_step): P = (1 - lr reg)^2
    cfg["max_gradient_norm"] = 1e3
    for s in range(2):
        m.train(None, batch_tuple(random_batch(cfg, B=16, Sn=2, seed=134 + s)[0]), 1.0)
    m._copt = copt
    cfg["max_gradient_norm"] = 0.05
    P = m.table_scale()
    assert abs(P - 0.95 ** 2) < 1e-6, P
    stored0 = m.get_params()                 # (the lazy optimizers never fold: the stored values)
    true = lambda d_, P_: {k: np.asarray(v, np.float64) * (P_ if k in orc.REG_TABLES else 1.0) for k, v in d_.items()}
    q0 = true(stored0, P)
    st["t"] = 2                              # (Adam's step count: the model's two steps so far)
    b = random_batch(cfg, B=20, Sn=2, seed=136)[0]
    loss, q, info, used = restricted_step(dict(q0), st, cat, b, cfg, 0.05, "adam", 0.05)
    l = m.train(None, batch_tuple(b), 0.05)
    assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (l, loss)
    assert m.table_scale() == P
    stored = m.get_params()
    got = true(stored, P)
    s1, s2 = m.get_slots()
    for k in q:
        if k.endswith("_b2"):
            continue
        a, r, r0 = (compared(k, np.asarray(x).reshape(np.shape(q[k])), used) for x in (got[k], q[k], q0[k]))
        assert np.abs(a - r).max() < 2e-3 * np.abs(r - r0).max() + 1e-6, k
        for gs, ref in ((s1[k], st["slot1"][k]), (s2[k], st["slot2"][k])):
            gs, ref = compared(k, np.asarray(gs).reshape(np.shape(ref)), used), compared(k, ref, used)
            assert np.abs(gs - ref).max() < 2e-3 * np.abs(ref).max() + 1e-9, k
    for k in ROW_TABLES:
        keep = ~used[k]
        assert np.array_equal(stored[k][keep], stored0[k][keep]), k


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
def test_lazy_sum_of_squares_and_scale(table_dtype):
    """Batches of varying B and Sn: St (state bytes 32..40) equals the tables' own fp64 sum of squares, P stays exactly 1,
    and two runs agree bit for bit in losses, parameters and slots."""
    import torch
    cfg = make_config(U=3000, I=4000, C=40, d=64, regulation_rate=0.05, max_gradient_norm=13.5, optimizer="lazy_adam")
    p = p32(random_params(cfg, seed=1401))
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = bf16_round(p[k]).astype(np.float64)
    _, cat = random_batch(cfg, B=8, Sn=2, seed=1400)
    shapes = [(64, 1), (5, 3), (40, 5), (1, 2), (64, 4), (17, 1)]
    batches = [batch_tuple(random_batch(cfg, B=B, Sn=Sn, seed=1410 + k)[0]) for k, (B, Sn) in enumerate(shapes)]
    probe = batch_tuple(random_batch(cfg, B=9, Sn=2, seed=1420)[0])
    runs = []
    for rep in range(2):
        m = model(cfg, cat, p, table_dtype=table_dtype)
        losses = [m.train(None, b, 0.01) for b in batches]
        m.grads(probe)                     # (folds the last step's records)
        St = float(m.state[32:40].view(torch.float64).item())
        ref = sum(float(getattr(m, k).double().pow(2).sum().item()) for k in orc.REG_TABLES)
        assert abs(St - ref) <= 1e-9 * ref, (St, ref)
        assert m.table_scale() == 1.0
        runs.append((losses, m.get_params(), m.get_slots()))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
        for j in range(2):
            assert np.array_equal(runs[0][2][j][k], runs[1][2][j][k]), k


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop", "adadelta"])
def test_lazy_optimizers_with_bf16_tables(optimizer):
    """bf16 tables: fp32 slots follow the restricted oracle, stored elements of used rows are one of the two bf16
    neighbours of the oracle's value, unused rows keep their bits, two runs leave the same bits."""
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer="lazy_" + optimizer)
    lr = {"adam": 0.01, "rmsprop": 0.01, "adadelta": 1.0}[optimizer]
    p = p32(random_params(cfg, seed=75))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    st = random_slots(p, optimizer, 76)
    b, cat = random_batch(cfg, B=36, Sn=3, seed=751)
    st0 = copy.deepcopy(st)
    loss, q, info, used = restricted_step(dict(p), st, cat, b, cfg, lr, optimizer, 0.05)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, [st0["slot1"], st0["slot2"]], table_dtype="bf16")
        l = m.train(None, batch_tuple(b), lr)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        outs.append((m.get_params(), m.get_slots()))
    got, (s1, s2) = outs[0]
    for k in q:
        assert np.array_equal(outs[0][0][k], outs[1][0][k]), k
        if k.endswith("_b2"):
            continue
        a, r = np.asarray(got[k], np.float64).reshape(q[k].shape), q[k]
        if k == "item_b":
            a, r = a[~used["item_b_amb"]], r[~used["item_b_amb"]]
        if k in BF16_TABLES:
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
            assert (np.abs(a - r) <= ulp * 1.001 + 2e-3 * np.abs(r - p[k]).max()).all(), k
            assert np.array_equal(a.astype(np.float32), bf16_round(a)), k
        else:
            step = np.abs(r - compared(k, p[k], used)).max()
            assert np.abs(a - r).max() < 2e-3 * step + 1e-7, k
        if k in used:
            keep = ~used[k]
            assert np.array_equal(a[keep], np.asarray(p[k])[keep]), k
        for gs, ref in ((s1[k], st["slot1"][k]), (s2[k], st["slot2"][k])):
            gs, ref = compared(k, np.asarray(gs).reshape(ref.shape), used), compared(k, ref, used)
            assert np.abs(gs - ref).max() < 2e-3 * np.abs(ref).max() + 1e-9, k


def test_lazy_adam_on_large_tables():
    """300 k users / 150 k items: the two-level scan and the sorted-user index; two steps against the restricted oracle."""
    cfg = make_config(U=300_000, I=150_000, C=40, d=64, regulation_rate=1e-3, max_gradient_norm=0.05,
                      optimizer="lazy_adam")
    p = p32(random_params(cfg, seed=85))
    st = orc.init_opt_state(p, "adam")
    _, cat = random_batch(cfg, B=4, Sn=2, seed=0)
    m = model(cfg, cat, p)
    q = dict(p)
    amb_all = []
    for s in range(2):
        b = random_batch(cfg, B=48, Sn=2 + s, seed=850 + s)[0]
        loss, q, info, used = restricted_step(q, st, cat, b, cfg, 0.05, "adam", 0.05)
        amb_all.append(used)
        l = m.train(None, batch_tuple(b), 0.05)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        sync_amb(m, q, st, used)
    got = m.get_params()
    s1, s2 = m.get_slots()
    amb = np.zeros(cfg["item_count"], bool)
    for u in amb_all:
        amb |= u["item_b_amb"]
    used = {"item_b_amb": amb}
    for k in q:
        if k.endswith("_b2"):
            continue
        a, r = compared(k, np.asarray(got[k]).reshape(q[k].shape), used), compared(k, q[k], used)
        assert np.abs(a - r).max() < 2e-3 * 2 * np.abs(r - compared(k, p[k], used)).max() + 1e-7, k
        for gs, ref in ((s1[k], st["slot1"][k]), (s2[k], st["slot2"][k])):
            gs, ref = compared(k, np.asarray(gs).reshape(ref.shape), used), compared(k, ref, used)
            assert np.abs(gs - ref).max() < 2e-3 * np.abs(ref).max() + 1e-9, k


def test_train_driver_with_lazy_adam(tmp_path):
    """--optimizer lazy_adam with the driver's default --l2_mode dense on the real Clothing tuples: 200 steps learn and
    the checkpoint carries both slots."""
    from tlsan_amd import train as T
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    args = T.parse(["--dataset", ds, "--max_steps", "200", "--eval_freq", "100", "--quiet", "--eval_topk", "0",
                    "--model_dir", str(tmp_path / "ck"), "--optimizer", "lazy_adam", "--learning_rate", "0.01"])
    res = T.train(args)
    assert res["steps"] == 200 and np.isfinite(res["final_auc"]) and 0.8 < res["final_auc"] < 1.0
    z = np.load(tmp_path / "ck" / "TLSAN-200.npz")
    assert int(z["global_step"]) == 200
    for s in ("slot1", "slot2"):
        assert any(f.startswith(s + "/") for f in z.files), z.files
        assert "%s/item_emb" % s in z.files and "%s/dense_K" % s in z.files

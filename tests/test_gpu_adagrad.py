"""Lazy Adagrad and row-wise Adagrad (TLSAN_OPT_ADAGRAD / TLSAN_OPT_ROWWISE_ADAGRAD with TLSAN_OPT_LAZY) on the GPU against
tests/adagrad_ref.py: TF 1.8's ApplyAdagrad on the oracle's clipped gradients, per element or with one accumulator per table
row, after which every row the batch did not use is put back, in W and in the accumulator.  Tolerances are those of
tests/test_gpu_lazy_opt.py: loss 2e-4 max(1, |loss|); used rows and dense weights 2e-3 (largest step of that parameter)
(steps so far) + 1e-7; accumulators 2e-3 max|ref| + 1e-9; unused rows and their accumulators bit for bit.  Starting
accumulators are random on every row (uniform(0.05, 0.5)), so that a sweep over unused rows would show."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests import adagrad_ref as ref
from tests.helpers import BF16_TABLES, batch_tuple, bf16_round, make_config, model, p32, random_batch, random_params
from tests.lazy_opt_ref import ROW_TABLES, SPARSE_CATEGORY_CASES, compared

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMENTWISE, ROWWISE = ref.KINDS
LR = 0.05


def sync_amb(m, q, acc, used):
    """carry the device's item_b (and its accumulator) of the saturated candidates into the reference for the next steps"""
    amb = used["item_b_amb"]
    if amb.any():
        q["item_b"] = np.where(amb, np.asarray(m.item_b.cpu().numpy(), np.float64), q["item_b"])
        acc["item_b"] = np.where(amb, np.asarray(m.get_slots()[0]["item_b"], np.float64), acc["item_b"])


def check_step(m, q, acc, p_prev, used, tol_n, exact_unused=None):
    got = m.get_params()
    slots = m.get_slots()
    assert len(slots) == 1
    s1 = slots[0]
    for k in q:
        assert np.shape(s1[k]) == np.shape(acc[k]), k
        if k.endswith("_b2"):
            continue      # (gradient = rounding noise, see test_gpu_parity.test_other_optimizers_track_oracle)
        a = compared(k, np.asarray(got[k], np.float64).reshape(np.shape(q[k])), used)
        r, r0 = compared(k, q[k], used), compared(k, p_prev[k], used)
        step = np.abs(r - r0).max()
        assert np.abs(a - r).max() < 2e-3 * step * tol_n + 1e-7, k
        gs, rs = compared(k, s1[k], used), compared(k, acc[k], used)
        assert np.abs(gs - rs).max() < 2e-3 * np.abs(rs).max() + 1e-9, k
    if exact_unused is not None:
        P0, S0 = exact_unused
        for k in ROW_TABLES:
            keep = ~used[k]
            assert np.array_equal(np.asarray(got[k], np.float32)[keep], np.asarray(P0[k], np.float32)[keep]), k
            assert np.array_equal(np.asarray(s1[k], np.float32)[keep], np.asarray(S0[0][k], np.float32)[keep]), k


@pytest.mark.parametrize("kind", ref.KINDS)
def test_adagrad_tracks_the_reference(kind, tmp_path):
    """Tables much larger than a batch: five clipped steps and one unclipped one, a checkpoint round trip in the middle.
    Loss, used rows and dense weights with their accumulators follow the reference; rows the step did not use keep W and
    their accumulator bit for bit."""
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer=kind,
                      model_dir=str(tmp_path))
    p = p32(random_params(cfg, seed=71))
    acc = ref.random_accumulators(p, kind, 72)
    _, cat = random_batch(cfg, B=8, Sn=3, seed=0)
    batches = [random_batch(cfg, B=16 + 4 * s, Sn=1 + s % 3, seed=700 + s)[0] for s in range(6)]
    m = model(cfg, cat, p, [acc])
    q = dict(p)
    for n, b in enumerate(batches):
        clip = 0.05 if n < 5 else 1e3
        m.config["max_gradient_norm"] = clip
        before = (m.get_params(), m.get_slots())
        prev = q
        loss, q, info, used = ref.restricted_adagrad_step(q, acc, cat, b, cfg, LR, kind, clip)
        assert (info["coef"] < 1.0) == (n < 5)
        l = m.train(None, batch_tuple(b), LR)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (n, l, loss)
        assert not used["user_emb"].all() and not used["item_emb"].all()
        check_step(m, q, acc, prev, used, n + 1, exact_unused=before)
        sync_amb(m, q, acc, used)
        if n == 2:                                # checkpoint round trip in the middle of the run
            path = m.save()
            m = model(cfg, cat, None)
            m.restore(None, path)
    assert m.table_scale() == 1.0


def test_restore_refuses_another_optimizers_slots(tmp_path):
    """A checkpoint whose slot shapes are not the model's optimizer's: a ValueError that names the slot's shape and the
    optimizer, and nothing is loaded."""
    cfg = make_config(U=30, I=45, C=5, d=64, optimizer=ELEMENTWISE, model_dir=str(tmp_path))
    _, cat = random_batch(cfg, B=4, Sn=1, seed=0)
    path = model(cfg, cat).save()
    m = model(dict(cfg, optimizer=ROWWISE), cat)
    before = m.get_params()
    with pytest.raises(ValueError) as e:
        m.restore(None, path)
    assert ROWWISE in str(e.value) and "(45, 32)" in str(e.value) and "(45,)" in str(e.value)
    with pytest.raises(ValueError):
        model(dict(cfg, optimizer="lazy_adam"), cat).restore(None, path)
    after = m.get_params()
    assert all(np.array_equal(before[k], after[k]) for k in before)


def _run(cfg, cat, kind, batches, clip=0.05, seed=80, table_dtype="f32", after_step=None):
    p = p32(random_params(cfg, seed=seed))
    acc = ref.random_accumulators(p, kind, seed + 1)
    m = model(dict(cfg, optimizer=kind), cat, p, [acc], table_dtype=table_dtype)
    q = dict(p)
    for s, b in enumerate(batches):
        before = (m.get_params(), m.get_slots())
        prev = q
        loss, q, info, used = ref.restricted_adagrad_step(q, acc, cat, b, cfg, LR, kind, clip)
        l = m.train(None, batch_tuple(b), LR)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (s, l, loss)
        check_step(m, q, acc, prev, used, s + 1, exact_unused=before)
        sync_amb(m, q, acc, used)
        if after_step is not None:
            after_step(b, used)


def _row_form_run(d, Ls, C, kind, B=24, Sn=3, steps=2, seed=80, U=200, I=300):
    cfg = make_config(U=U, I=I, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=0.05)
    _, cat = random_batch(cfg, B=8, Sn=2, seed=seed + 2)
    _run(cfg, cat, kind, [random_batch(cfg, B=B, Sn=Sn, seed=seed + 10 + s)[0] for s in range(steps)], seed=seed)


ROW_FORMS = [(64, 10, 20, 24), (128, 10, 20, 24), (256, 10, 20, 24), (128, 90, 20, 24), (256, 90, 12, 24), (64, 10, 2, 96)]


@pytest.mark.parametrize("d,Ls,C,B,kind", [f + (ROWWISE,) for f in ROW_FORMS] +
                         [f + (ELEMENTWISE,) for f in ROW_FORMS if f[:3] in ((128, 10, 20), (256, 90, 12), (64, 10, 2))])
def test_adagrad_row_forms(d, Ls, C, B, kind):
    """Narrow and wide rows -- d_i = 32 leaves half of a row's 16 lanes empty, d = 256 takes two chunks a lane --, the
    usert_emb tail at Ls = 10 and 90 (no multiples of 4), and two large categories that several row-sum workgroups share
    (the Rc64 sums the row update clears)."""
    _row_form_run(d, Ls, C, kind, B=B)


def test_row_accumulator_is_a_row_mean():
    """One unclipped step at d = 128: for every used row of the four tables acc' - acc is the mean of the row's squared
    gradients, relative 2e-3 -- beside the rounding of acc' itself, one fp32 ulp, which the difference inherits -- and the
    row moved by ONE factor, -lr / sqrt(acc'), times its gradient: 2e-3 of the row's largest step beside the fp32 rounding of
    the stored elements."""
    kind = ROWWISE
    cfg = make_config(U=200, I=300, C=20, d=128, Ls=10, regulation_rate=1e-3, max_gradient_norm=1e3, optimizer=kind)
    p = p32(random_params(cfg, seed=90))
    acc = ref.random_accumulators(p, kind, 91)
    acc0 = {k: v.copy() for k, v in acc.items()}
    b, cat = random_batch(cfg, B=24, Sn=3, seed=92)
    m = model(cfg, cat, p, [acc])
    loss, q, info, used = ref.restricted_adagrad_step(dict(p), acc, cat, b, cfg, LR, kind, 1e3)
    l = m.train(None, batch_tuple(b), LR)
    assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
    got, s1 = m.get_params(), m.get_slots()[0]
    eps = 2.0 ** -23
    for k in ref.ROW_KEYS:
        rows = used[k]
        assert rows.any(), k
        g = info["g"][k][rows]
        mean_sq = (g * g).mean(axis=1)
        a1 = np.asarray(s1[k], np.float64)[rows]
        d_acc = a1 - acc0[k][rows]
        assert mean_sq.max() > 1e3 * eps, k        # (the increments are well above the accumulators' resolution)
        assert (np.abs(d_acc - mean_sq) <= 2e-3 * mean_sq + eps * a1).all(), k
        w0, w1 = p[k][rows], np.asarray(got[k], np.float64)[rows]
        want = (-LR / np.sqrt(a1))[:, None] * g
        tol = 2e-3 * np.abs(want).max(axis=1, keepdims=True) + eps * np.maximum(np.abs(w0), np.abs(w1))
        assert (np.abs((w1 - w0) - want) <= tol).all(), k


def test_width_one_parameters_agree_between_the_kinds():
    """From the same parameters with every accumulator at 0.1 (what Model allocates), one step of each kind: item_b and
    every dense weight -- width 1, the elementwise rule in both -- come out bit-equal, with their accumulators."""
    cfg = make_config(U=200, I=300, C=20, d=64, regulation_rate=1e-3, max_gradient_norm=0.05)
    p = p32(random_params(cfg, seed=93))
    b, cat = random_batch(cfg, B=24, Sn=3, seed=94)
    out = []
    for kind in ref.KINDS:
        m = model(dict(cfg, optimizer=kind), cat, p)
        s0 = m.get_slots()
        assert len(s0) == 1 and all(np.all(v == np.float32(0.1)) for v in s0[0].values())
        assert s0[0]["item_emb"].shape == ((300,) if kind == ROWWISE else (300, 32))
        m.train(None, batch_tuple(b), LR)
        out.append((m.get_params(), m.get_slots()[0]))
    (pe, se), (pr, sr) = out
    moved = 0
    for k in pe:
        if k in ref.ROW_KEYS:
            continue
        assert np.array_equal(pe[k], pr[k]) and np.array_equal(se[k], sr[k]), k
        moved += int((np.asarray(pe[k], np.float32) != np.asarray(p[k], np.float32)).sum())
    assert moved > 0


def _sparse_category_run(kind, C, item_cates, ucate_cates, B, d=64, Ls=10, steps=2, seed=120):
    """_sparse_category_run of tests/test_gpu_lazy_opt.py: some categories are reached only through items, some named only
    by u_cate, the rest are unused and keep W and their accumulator bit for bit."""
    cfg = make_config(U=300, I=450, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=0.05)
    rng = np.random.RandomState(seed)
    cat = rng.choice(np.asarray(item_cates), cfg["item_count"]).astype(np.int32)
    batches = []
    for s in range(steps):
        b = random_batch(cfg, B=B, Sn=3, seed=seed + 10 + s)[0]
        b["u_cate"] = rng.choice(np.asarray(ucate_cates), B).astype(np.int64)
        batches.append(b)
    count = dict(only_items=0, only_ucate=0, unused=0)

    def tally(b, used):
        by_item = np.zeros(C, bool)
        by_item[cat[used["item_emb"]]] = True
        by_ucate = np.zeros(C, bool)
        by_ucate[b["u_cate"]] = True
        count["only_items"] += int((by_item & ~by_ucate).sum())
        count["only_ucate"] += int((by_ucate & ~by_item).sum())
        count["unused"] += int((~used["cate_emb"]).sum())

    _run(cfg, cat, kind, batches, seed=seed + 1, after_step=tally)
    assert min(count.values()) > 0, count


@pytest.mark.parametrize("C,item_cates,ucate_cates,B,d", [c[1:] for c in SPARSE_CATEGORY_CASES])
def test_rowwise_adagrad_leaves_unused_category_rows_alone(C, item_cates, ucate_cates, B, d):
    _sparse_category_run(ROWWISE, C, item_cates, ucate_cates, B, d=d)


_CSEG = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_adagrad import ROWWISE, _row_form_run, _sparse_category_run
from tests.lazy_opt_ref import SPARSE_CATEGORY_CASES
_row_form_run(64, 10, 40, ROWWISE, B=32, seed=90)
_row_form_run(128, 24, 40, ROWWISE, B=32, seed=91)
for _, C, item_cates, ucate_cates, B, d in SPARSE_CATEGORY_CASES:
    _sparse_category_run(ROWWISE, C, item_cates, ucate_cates, B, d=d, seed=140)
print("ok")
"""


def test_rowwise_adagrad_with_category_segments():
    """Category segments (TLSAN_CSEG_MIN=1 in a child process: read once per process), the sparse category tables
    included: a category's segment then counts every use."""
    env = dict(os.environ, TLSAN_CSEG_MIN="1")
    r = subprocess.run([sys.executable, "-c", _CSEG, ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_rowwise_adagrad_on_a_scaled_state():
    """test_lazy_step_on_a_scaled_state's protocol: two unclipped lazy-L2 SGD steps at reg 0.05 leave P = 0.95^2; the
    row-wise step then acts on the true values P * stored and leaves P as it is."""
    kind = ROWWISE
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=0.05, max_gradient_norm=0.05, optimizer=kind)
    p = p32(random_params(cfg, seed=131))
    acc = ref.random_accumulators(p, kind, 132)
    _, cat = random_batch(cfg, B=8, Sn=3, seed=133)
    m = model(cfg, cat, p, [acc])
    copt, m._copt = m._copt, None            # two unclipped lazy-L2 SGD steps (tlsan_train_step): P = (1 - lr reg)^2
    cfg["max_gradient_norm"] = 1e3
    for s in range(2):
        m.train(None, batch_tuple(random_batch(cfg, B=16, Sn=2, seed=134 + s)[0]), 1.0)
    m._copt = copt
    cfg["max_gradient_norm"] = 0.05
    P = m.table_scale()
    assert abs(P - 0.95 ** 2) < 1e-6, P
    stored0 = m.get_params()                 # (the lazy optimizers never fold: the stored values)
    slots0 = m.get_slots()[0]
    true = lambda d_, P_: {k: np.asarray(v, np.float64) * (P_ if k in orc.REG_TABLES else 1.0) for k, v in d_.items()}
    q0 = true(stored0, P)
    b = random_batch(cfg, B=20, Sn=2, seed=136)[0]
    loss, q, info, used = ref.restricted_adagrad_step(dict(q0), acc, cat, b, cfg, LR, kind, 0.05)
    l = m.train(None, batch_tuple(b), LR)
    assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (l, loss)
    assert m.table_scale() == P
    stored = m.get_params()
    got = true(stored, P)
    s1 = m.get_slots()[0]
    for k in q:
        if k.endswith("_b2"):
            continue
        a, r, r0 = (compared(k, np.asarray(x).reshape(np.shape(q[k])), used) for x in (got[k], q[k], q0[k]))
        assert np.abs(a - r).max() < 2e-3 * np.abs(r - r0).max() + 1e-6, k
        gs, rs = compared(k, s1[k], used), compared(k, acc[k], used)
        assert np.abs(gs - rs).max() < 2e-3 * np.abs(rs).max() + 1e-9, k
    for k in ROW_TABLES:
        keep = ~used[k]
        assert np.array_equal(stored[k][keep], stored0[k][keep]), k
        assert np.array_equal(s1[k][keep], slots0[k][keep]), k


@pytest.mark.parametrize("kind", ref.KINDS)
def test_adagrad_with_bf16_tables(kind):
    """bf16 tables: the fp32 accumulators follow the reference, stored elements of used rows are within one bf16 ulp (plus
    2e-3 of the step) of the reference's value and representable in bf16, unused rows keep their bits, two runs leave the
    same bits."""
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer=kind)
    p = p32(random_params(cfg, seed=75))
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    acc = ref.random_accumulators(p, kind, 76)
    acc0 = {k: v.copy() for k, v in acc.items()}
    b, cat = random_batch(cfg, B=36, Sn=3, seed=751)
    loss, q, info, used = ref.restricted_adagrad_step(dict(p), acc, cat, b, cfg, LR, kind, 0.05)
    outs = []
    for rep in range(2):
        m = model(cfg, cat, p, [acc0], table_dtype="bf16")
        l = m.train(None, batch_tuple(b), LR)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        outs.append((m.get_params(), m.get_slots()[0]))
    got, s1 = outs[0]
    for k in q:
        assert np.array_equal(outs[0][0][k], outs[1][0][k]), k
        assert np.array_equal(outs[0][1][k], outs[1][1][k]), k
        if k.endswith("_b2"):
            continue
        full = np.asarray(got[k], np.float64).reshape(q[k].shape)
        a, r = compared(k, full, used), compared(k, q[k], used)
        if k in BF16_TABLES:
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 1e-30))) - 7)
            assert (np.abs(a - r) <= ulp * 1.001 + 2e-3 * np.abs(r - p[k]).max()).all(), k
            assert np.array_equal(a.astype(np.float32), bf16_round(a)), k
        else:
            step = np.abs(r - compared(k, p[k], used)).max()
            assert np.abs(a - r).max() < 2e-3 * step + 1e-7, k
        if k in used:
            keep = ~used[k]
            assert np.array_equal(full[keep], np.asarray(p[k])[keep]), k
            assert np.array_equal(np.asarray(s1[k], np.float32)[keep], np.asarray(acc0[k], np.float32)[keep]), k
        gs, rs = compared(k, s1[k], used), compared(k, acc[k], used)
        assert np.abs(gs - rs).max() < 2e-3 * np.abs(rs).max() + 1e-9, k


@pytest.mark.parametrize("kind,table_dtype", [(ROWWISE, "f32"), (ROWWISE, "bf16"), (ELEMENTWISE, "f32"), (ELEMENTWISE, "bf16")])
def test_adagrad_sum_of_squares_and_scale(kind, table_dtype):
    """Batches of varying B and Sn: St (state bytes 32..40) equals the tables' own fp64 sum of squares, P stays exactly 1,
    and two runs agree bit for bit in losses, parameters and accumulators."""
    import torch
    cfg = make_config(U=3000, I=4000, C=40, d=64, regulation_rate=0.05, max_gradient_norm=13.5, optimizer=kind)
    p = p32(random_params(cfg, seed=1401))
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = bf16_round(p[k]).astype(np.float64)
    acc = ref.random_accumulators(p, kind, 1402)
    _, cat = random_batch(cfg, B=8, Sn=2, seed=1400)
    shapes = [(64, 1), (5, 3), (40, 5), (1, 2), (64, 4), (17, 1)]
    batches = [batch_tuple(random_batch(cfg, B=B, Sn=Sn, seed=1410 + k)[0]) for k, (B, Sn) in enumerate(shapes)]
    probe = batch_tuple(random_batch(cfg, B=9, Sn=2, seed=1420)[0])
    runs = []
    for rep in range(2):
        m = model(cfg, cat, p, [acc], table_dtype=table_dtype)
        losses = [m.train(None, b, LR) for b in batches]
        m.grads(probe)                     # (folds the last step's records)
        St = float(m.state[32:40].view(torch.float64).item())
        want = sum(float(getattr(m, k).double().pow(2).sum().item()) for k in orc.REG_TABLES)
        assert abs(St - want) <= 1e-9 * want, (St, want)
        assert m.table_scale() == 1.0
        runs.append((losses, m.get_params(), m.get_slots()[0]))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
        assert np.array_equal(runs[0][2][k], runs[1][2][k]), k
    assert any(not np.array_equal(runs[0][2][k], np.asarray(acc[k], np.float32)) for k in ref.ROW_KEYS)


def test_rowwise_adagrad_on_large_tables():
    """300 k users / 150 k items: the two-level scan and the sorted-user index; two steps from accumulators at 0.1 against
    the reference."""
    kind = ROWWISE
    cfg = make_config(U=300_000, I=150_000, C=40, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer=kind)
    p = p32(random_params(cfg, seed=85))
    acc = ref.initial_accumulators(p, kind)
    _, cat = random_batch(cfg, B=4, Sn=2, seed=0)
    m = model(cfg, cat, p)
    q = dict(p)
    amb = np.zeros(cfg["item_count"], bool)
    for s in range(2):
        b = random_batch(cfg, B=48, Sn=2 + s, seed=850 + s)[0]
        loss, q, info, used = ref.restricted_adagrad_step(q, acc, cat, b, cfg, LR, kind, 0.05)
        amb |= used["item_b_amb"]
        l = m.train(None, batch_tuple(b), LR)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss))
        sync_amb(m, q, acc, used)
    got = m.get_params()
    s1 = m.get_slots()[0]
    used = {"item_b_amb": amb}
    for k in q:
        if k.endswith("_b2"):
            continue
        a, r = compared(k, np.asarray(got[k]).reshape(q[k].shape), used), compared(k, q[k], used)
        assert np.abs(a - r).max() < 2e-3 * 2 * np.abs(r - compared(k, p[k], used)).max() + 1e-7, k
        gs, rs = compared(k, s1[k], used), compared(k, acc[k], used)
        assert np.abs(gs - rs).max() < 2e-3 * np.abs(rs).max() + 1e-9, k


def test_train_driver_with_lazy_rowwise_adagrad(tmp_path):
    """--optimizer lazy_rowwise_adagrad with the driver's default --l2_mode dense on the real Clothing tuples: 200 steps
    learn and the checkpoint carries one slot set with one float per table row."""
    from tlsan_amd import train as T
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    args = T.parse(["--dataset", ds, "--max_steps", "200", "--eval_freq", "100", "--quiet", "--eval_topk", "0",
                    "--model_dir", str(tmp_path / "ck"), "--optimizer", "lazy_rowwise_adagrad", "--learning_rate", "0.05"])
    res = T.train(args)
    print("final_auc", res["final_auc"])
    assert res["steps"] == 200 and np.isfinite(res["final_auc"]) and 0.5 < res["final_auc"] < 1.0
    z = np.load(tmp_path / "ck" / "TLSAN-200.npz")
    assert int(z["global_step"]) == 200
    assert z["slot1/item_emb"].shape == (z["item_emb"].shape[0],) and z["slot1/cate_emb"].shape == (z["cate_emb"].shape[0],)
    assert "slot1/dense_K" in z.files and not any(f.startswith("slot2/") for f in z.files), z.files

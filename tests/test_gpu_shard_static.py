"""Static-shape sharded step (ShardedModel(static_rows=...), include/tlsan.h tlsan_*_static): the same numbers, bit for
bit, as the step whose exchange sizes pass through the host -- eagerly with one or two batches announced ahead, replayed
from HIP graphs, over two ranks -- and a loud failure when a batch does not fit the fixed exchange."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import bf16_round
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu


def _one_rank_worker(rank, world):
    from tlsan_amd import synth
    from tlsan_amd.dist import ShardedModel
    cfg = synth.make_config("electronics", user_count=3001, item_count=2203, cate_count=67)
    icl = synth.item_cate_list(cfg)
    batches = synth.make_batches(cfg, 4, 512, seed=5, sessions="amazon")
    N = 12

    def run(static, ahead, graphs=False):
        m = ShardedModel(cfg, icl, device="cuda:0", l2_mode="lazy", static_rows=static)
        dbs = [m.device_batch(b) for b in batches]
        losses = []
        nb = lambda s, j: dbs[(s + j) % 4] if ahead >= j else None
        n_eager = 4 if graphs else N
        for s in range(n_eager):
            kw = dict(after_next=nb(s, 2)) if static else {}
            m.train_async(dbs[s % 4], 0.7, next_batch=nb(s, 1), **kw)
            losses.append(float(m.last_loss.item()))
        if graphs:
            gs = []
            for i in range(4):            # capture and replay alternately along the cycle
                g = m.capture_step(dbs[i], dbs[(i + 1) % 4], 0.7)
                m.replay(g)
                losses.append(float(m.last_loss.item()))
                gs.append(g)
            for s in range(8, N):
                m.replay(gs[s % 4])
                losses.append(float(m.last_loss.item()))
        if static:
            m.check_static_overflow()
        return losses, m.gather_params()

    l0, p0 = run(False, 1)
    for name, args in (("static, one ahead", (True, 1)), ("static, two ahead", (True, 2)), ("static, none ahead", (True, 0)),
                       ("static, fixed capacity", (2560, 2)), ("static, graphs", (True, 1, True)),
                       # (the eager steps leave a plan for the batch after next in the slot the first graph plans into)
                       ("static, graphs behind steps that announced two ahead", (True, 2, True))):
        l1, p1 = run(*args)
        assert l1 == l0, (name, l0, l1)
        for k in p0:
            assert np.array_equal(p0[k], p1[k]), (name, k)

    # an announcement that is not honoured: the plans built for it are taken out of their slots again (their
    # destination index is counted into the slot's state; a second plan on top of it would double every count)
    order = [0, 3, 1, 2, 0, 1]

    def run_order(static):
        m = ShardedModel(cfg, icl, device="cuda:0", l2_mode="lazy", static_rows=static)
        dbs = [m.device_batch(b) for b in batches]
        losses = []
        for i, k in enumerate(order):
            kw = {}
            if static and i == 0:
                kw = dict(next_batch=dbs[1], after_next=dbs[2])     # ... and then batch 3 is trained
            m.train_async(dbs[k], 0.7, **kw)
            losses.append(float(m.last_loss.item()))
        if static:
            m.check_static_overflow()
        return losses, m.gather_params()

    la, pa = run_order(False)
    lb, pb = run_order(True)
    assert la == lb, ("abandoned announcement", la, lb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), ("abandoned announcement", k)

    # steps that announce nothing followed by a step that announces two batches, with the GPU's queue running behind the
    # host (no loss is read until the end): the plans of the announcing step go to slots that the two steps before it
    # used last, so they may only be issued once the step before has STARTED -- which the pinned word can only tell if
    # that step, too, carried a stamp (before, only announcing steps stamped, and the plan was ordered behind
    # the step before the silent ones).  Same numbers as the dynamic step, bit for bit.
    def run_gaps(static):
        m = ShardedModel(cfg, icl, device="cuda:0", l2_mode="lazy", static_rows=static)
        dbs = [m.device_batch(b) for b in batches]
        losses = []
        for s in range(24):
            silent = s % 6 in (3, 4)                      # two silent steps, then one that announces two ahead
            kw = {}
            if not silent:
                kw = dict(next_batch=dbs[(s + 1) % 4])
                if static:
                    kw["after_next"] = dbs[(s + 2) % 4]
            m.train_async(dbs[s % 4], 0.7, **kw)
            losses.append(m.last_loss.clone())
        if static:
            m.check_static_overflow()
        return [float(l.item()) for l in losses], m.gather_params()

    lg0, pg0 = run_gaps(False)
    lg1, pg1 = run_gaps(True)
    assert lg0 == lg1, ("silent steps before an announcing one", lg0, lg1)
    for k in pg0:
        assert np.array_equal(pg0[k], pg1[k]), ("silent steps before an announcing one", k)

    # a batch that needs more rows of an owner than the exchange holds is reported, not silently truncated
    m = ShardedModel(cfg, icl, device="cuda:0", l2_mode="lazy", static_rows=64)
    m.train_async(m.device_batch(batches[0]), 0.7)
    try:
        m.check_static_overflow()
        raise AssertionError("overflow not reported")
    except RuntimeError as e:
        assert "static_rows" in str(e)
    try:
        ShardedModel(cfg, icl, device="cuda:0", l2_mode="dense", static_rows=True)
        raise AssertionError("dense + static accepted")
    except NotImplementedError:
        pass


def test_static_step_equals_dynamic_step_at_one_rank():
    run_ranks(_one_rank_worker, 1, timeout=600)


def _moved_branches_worker(rank, world):
    import tempfile
    from tlsan_amd import synth
    from tlsan_amd.dist import ShardedModel
    base = synth.make_config("electronics", user_count=3001, item_count=2203, cate_count=67)
    icl = synth.item_cate_list(base)
    batches = synth.make_batches(base, 4, 256, seed=5, sessions="amazon")
    test_batch = synth.make_batches(base, 1, 64, seed=5, test=True, sessions="amazon")[0]
    weights = (1.0, 0.5, 1.0, 0.25)

    def run(static, model_dir):
        m = ShardedModel(dict(base, model_dir=model_dir), icl, device="cuda:0", l2_mode="lazy", static_rows=static)
        dbs = [m.device_batch(b) for b in batches]
        losses, ranks = [], None
        for s in range(8):
            kw = dict(after_next=dbs[(s + 2) % 4]) if static else {}
            m.train_async(dbs[s % 4], 0.7, next_batch=dbs[(s + 1) % 4], weight=weights[s % 4], **kw)
            losses.append(float(m.last_loss.item()))
            if s + 1 == 3:        # an evaluation between steps whose successors' plans are announced
                ranks = m.label_ranks(test_batch).cpu().numpy()
            if s + 1 == 5:        # a restore in mid-run, with announced plans outstanding
                m.restore(None, m.save(sharded=True))
        if static:
            m.check_static_overflow()
        return losses, ranks, m.gather_params()

    with tempfile.TemporaryDirectory() as tmp:
        l0, r0, p0 = run(False, os.path.join(tmp, "dynamic"))
        l1, r1, p1 = run(True, os.path.join(tmp, "static"))
    assert r0.shape == (64,) and np.array_equal(r0, r1), ("label ranks", r0, r1)
    assert l1 == l0, ("losses", l0, l1)
    for k in p0:
        assert np.array_equal(p0[k], p1[k]), k


def test_static_step_with_weights_evaluation_and_restore_equals_dynamic_step():
    """The static step where the steps' weights differ from 1, with an evaluation and a save / restore between steps
    that have announced both successors: the same losses, label ranks and parameters as the dynamic step, bit for bit."""
    run_ranks(_moved_branches_worker, 1, timeout=600)


def _two_rank_worker(rank, world):
    from tlsan_amd import synth
    from tlsan_amd.dist import ShardedModel
    cfg = synth.make_config("electronics", user_count=3001, item_count=2203, cate_count=67)
    icl = synth.item_cate_list(cfg)
    per_step = [[synth.make_batches(cfg, 1, 256, seed=700 + 10 * s + r, sessions="amazon")[0] for r in range(world)] for s in range(4)]

    def run(static, ahead, deferred=False, graphs=False, coalesce=False):
        m = ShardedModel(cfg, icl, device="cuda:0", l2_mode="lazy", static_rows=static, deferred_ids=deferred, coalesce=coalesce)
        dbs = [m.device_batch(per[rank]) for per in per_step]
        losses = []
        if graphs:      # one eager step, then the cycle of four recorded steps, replayed: 2 + 4 = the six steps below
            m.train_async(dbs[0], 0.7, next_batch=dbs[1])
            losses.append(float(m.last_loss.item()))
            gs = []
            for i in range(4):
                g = m.capture_step(dbs[(1 + i) % 4], dbs[(2 + i) % 4], 0.7)
                m.replay(g)
                losses.append(float(m.last_loss.item()))
                gs.append(g)
            m.replay(gs[0])
            losses.append(float(m.last_loss.item()))
        else:
            for s in range(6):
                nb = lambda j: dbs[(s + j) % 4] if ahead >= j else None
                kw = dict(after_next=nb(2)) if static else {}
                m.train_async(dbs[s % 4], 0.7, next_batch=nb(1), **kw)
                losses.append(float(m.last_loss.item()))
        if static:
            m.check_static_overflow()
        return losses, m.gather_params()

    l0, p0 = run(False, 1)
    # (deferred: plans built ahead leave their id exchange to the step that uses them -- what runs by default over RCCL,
    #  where no second communicator is opened.  Recorded steps cannot be part of this test: gloo's exchange is staged
    #  through the host, which a stream capture cannot hold; test_sharded_step_over_rccl replays graphs where there
    #  are two GPUs.)
    # (coalesce: the row gradients' all-to-all issued with the all-reduce, AHEAD of the summary -- under gloo as two
    #  staged calls back to back: the order of the step's phases is what is under test)
    for args in ((True, 1), (True, 2), (True, 1, True), (True, 2, True), (True, 2, False, False, True), (True, 1, True, False, True)):
        l1, p1 = run(*args)
        assert l1 == l0, (args, l0, l1)
        for k in p0:
            assert np.array_equal(p0[k], p1[k]), (args, k)


def test_static_step_equals_dynamic_step_over_two_ranks():
    """Two processes on one GPU (gloo stages the collectives through the host): the equal-split exchange of the static
    step against the sized one, rows owned by the other rank included."""
    run_ranks(_two_rank_worker, 2, timeout=600)


def test_side_streams_run_beside_the_main_stream():
    """model.concurrent_streams: the streams it returns overlap work on the current stream and on each other (HIP
    multiplexes streams onto a few hardware queues; two streams on one queue execute like one)."""
    from tlsan_amd.model import concurrent_streams
    dev = torch.device("cuda:0")
    streams = concurrent_streams(dev, 2)
    assert len(streams) == 2 and streams[0] is not streams[1]
    main = torch.cuda.current_stream(dev)
    x = torch.zeros(64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for a, b in ((main, streams[0]), (main, streams[1]), (streams[0], streams[1])):
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(a):
            ev[0].record(a)
            torch.cuda._sleep(2000000)           # ~1 ms of spinning on a
            ev[1].record(a)
        with torch.cuda.stream(b):
            x.add_(1.0)                          # launched after it, on b
            ev[2].record(b)
        torch.cuda.synchronize(dev)
        assert ev[0].elapsed_time(ev[2]) < 0.5 * ev[0].elapsed_time(ev[1]), "the tiny kernel waited for the spin: one queue"


def _wire_worker(rank, world):
    from oracle import tlsan_oracle as orc
    from tests.helpers import make_config, random_batch, random_params
    from tlsan_amd.dist import ShardedModel
    reg = 1e-3
    cfg = make_config(U=61, I=83, C=9, d=128, regulation_rate=reg)
    p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in random_params(cfg, seed=17).items()}
    _, cat = random_batch(cfg, B=4, Sn=2, seed=0)
    tup = lambda b: (b["u"], b["i"], b["y"], b["hist_i"], b["hist_i_new"], b["hist_t"], b["sl"], b["sl_new"], b["u_cate"])
    steps = [[random_batch(cfg, B=24, Sn=3, seed=2000 + 10 * s + r)[0] for r in range(world)] for s in range(3)]
    m = ShardedModel(cfg, cat, device="cuda:0", l2_mode="lazy", static_rows=True, wire_dtype="bf16")
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    dbs = [m.device_batch(tup(per[rank])) for per in steps]
    losses = []
    for k, db in enumerate(dbs):
        m.train_async(db, 0.8, next_batch=dbs[k + 1] if k + 1 < len(dbs) else None)
        losses.append(float(m.last_loss.item()))
    m.check_static_overflow()
    got = m.gather_params()
    if rank == 0:
        # the same steps on the CPU: forward / backward at the bf16-rounded embedding tables, L2 term, clip norm and
        # update on the fp32 weights the owners keep
        q, ref, P = dict(p), [], 1.0        # P: the lazy-L2 table scale (tables = P * stored; what is rounded is `stored`)
        for per in steps:
            Sn = max(b["hist_i_new"].shape[1] for b in per)
            g_b = {k: np.concatenate([np.pad(b[k], ((0, 0), (0, Sn - b[k].shape[1]))) if k == "hist_i_new" else b[k]
                                      for b in per], 0) for k in per[0]}
            qr = dict(q)
            for k in ("item_emb", "user_emb", "cate_emb"):
                qr[k] = bf16_round(q[k] / P).astype(np.float64) * P
            bce, _, g, sparse = orc.backward(qr, cat, g_b, 8, 0.0)
            for k in orc.REG_TABLES:
                g[k] = sparse["g_sparse"][k] + reg * q[k]
            norm = orc.global_norm(q, g, sparse, reg, "tf18")
            coef = 5.0 / max(norm, 5.0)
            ref.append(bce + reg * orc.l2_term(q))
            q = {k: q[k] - 0.8 * coef * g[k] for k in q}
            P *= 1.0 - 0.8 * coef * reg
        assert np.allclose(losses, ref, rtol=3e-4, atol=1e-5), (losses, ref)
        for k in q:
            du = np.asarray(got[k], np.float64).reshape(q[k].shape) - p[k]
            dr = q[k] - p[k]
            # (a value within fp32 rounding of a bf16 tie may round the other way here than on the GPU: one such
            #  element moves a few gradient rows by 2^-8 of themselves)
            assert np.abs(du - dr).max() < 5e-3 * (np.abs(dr).max() + 1e-9) + 1e-6, (k, float(np.abs(du - dr).max()), float(np.abs(dr).max()))


@pytest.mark.parametrize("world", [1, 2])
def test_bf16_rows_on_the_wire(world):
    """ShardedModel(wire_dtype="bf16"): owners keep fp32 rows, the copies the kernels gather from carry bf16 embedding
    values.  Against the oracle run the same way: gradients at the rounded tables, L2 / clip / update on the fp32 ones."""
    run_ranks(_wire_worker, world, timeout=600)

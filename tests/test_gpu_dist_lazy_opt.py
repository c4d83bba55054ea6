"""Lazy Adam / RMSProp / Adadelta on the row-sharded step (ShardedModel(l2_mode="lazy"), tlsan_shard_apply_lazy_opt)
against the restricted oracle of tests/lazy_opt_ref.py on the concatenated batch: the dense optimizer's step with
every row the GLOBAL batch did not use put back, in W and both slots.  Two processes share cuda:0 and talk over gloo, as
in tests/test_gpu_dist.py."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.helpers import batch_tuple, concat_batches, make_config, p32, random_batch, random_params, sharded
from tests.lazy_opt_ref import (LR, ROW_TABLES, check_step, cover_all_batch, driver_worker, random_slots, restricted_step,
                                sync_amb, used_rows)
from tests.ranks import run_ranks
from tests.shard_ref import _np_opt_elem

pytestmark = pytest.mark.gpu


class _AsModel:
    """what check_step and sync_amb ask of a model, answered by a ShardedModel (collectives: every rank calls them)"""

    def __init__(self, m):
        self.m = m

    def get_params(self):
        return self.m.gather_params()

    def get_slots(self):
        return self.m.gather_slots()

    @property
    def item_b(self):
        return torch.as_tensor(self.m.gather_params()["item_b"])


def _oracle_batches(cfg, world):
    """Six global batches, 16 + 4 s samples per rank, session lengths that differ between the ranks; with two ranks the
    first user and the first candidate of rank 1 are rank 0's, so that some rows are sent by both.  u_cate names the
    categories 0..17 and the items belong to 0..16 (_oracle_run), so that of the 20 categories one is reached by u_cate
    alone and two by nothing: a global batch of this size would otherwise use every category."""
    steps = []
    for s in range(6):
        per = [random_batch(cfg, B=16 + 4 * s, Sn=1 + (s + r) % 3, seed=700 + 10 * s + r)[0] for r in range(world)]
        for b in per:
            b["u_cate"] %= 18
        if world > 1:
            per[1]["u"][0] = per[0]["u"][0]
            per[1]["i"][0] = per[0]["i"][0]
        steps.append(per)
    return steps


def _oracle_run(rank, world, optimizer, reg, ckpt):
    """The six steps against the restricted oracle: returns (losses, parameters, slots, model, cfg, cat, _sq) of the end
    of the sixth (the model itself is then taken back to step 3, see the end)."""
    cfg = make_config(U=300, I=450, C=20, d=64, regulation_rate=reg, max_gradient_norm=0.05,
                      optimizer="lazy_" + optimizer, model_dir=ckpt)
    lr = LR[optimizer]
    p = p32(random_params(cfg, seed=71))
    st = random_slots(p, optimizer, 72)
    cat = np.random.RandomState(70).randint(0, 17, cfg["item_count"]).astype(np.int32)
    m = sharded(cfg, cat, p, [st["slot1"], st["slot2"]])
    q = dict(p)
    losses, prefix = [], None
    for n, per in enumerate(_oracle_batches(cfg, world)):
        clip = 0.05 if n < 5 else 1e3
        m.clip = clip
        if world > 1:      # rows both ranks send, rows one rank sends: the sum over the sources and the ownership rule
            u0, u1 = (used_rows(b, cat, cfg) for b in per)
            for k in ("user_emb", "item_emb"):
                assert (u0[k] & u1[k]).any() and (u0[k] ^ u1[k]).any(), k
        before = (m.gather_params(), m.gather_slots())
        prev = q
        loss, q, info, used = restricted_step(q, st, cat, concat_batches(per), cfg, lr, optimizer, clip)
        assert (info["coef"] < 1.0) == (n < 5)
        for k in ROW_TABLES:
            assert not used[k].all(), k
        m.train_async(batch_tuple(per[rank]), lr)
        l = float(m.last_loss.item())
        losses.append(l)
        assert abs(l - loss) < 2e-4 * max(1.0, abs(loss)), (n, l, loss)
        check_step(_AsModel(m), q, st, prev, used, n + 1, exact_unused=before)
        sync_amb(_AsModel(m), q, st, used)
        if n == 2:       # checkpoint round trips in the middle of the run: the per-rank files, and the gathered single file
            want = (m.gather_params(), m.gather_slots())
            prefix = m.save()
            for path in (prefix, m.save(sharded=False) + ".npz"):
                m2 = sharded(dict(cfg), cat, seed=99)
                m2.restore(None, path)
                assert m2.global_step.eval() == 3
                back = (m2.gather_params(), m2.gather_slots())
                for k in want[0]:
                    assert np.array_equal(back[0][k], want[0][k]), (path, k)
                    for j in range(2):
                        assert np.array_equal(back[1][j][k], want[1][j][k]), (path, j, k)
            m = m2       # (the model restored from the single file trains on)
    assert float(m._P.item()) == 1.0
    out = (losses, m.gather_params(), m.gather_slots(), m, cfg, cat, (float(m._sq[0].item()), float(m._sq[1].item())))
    # back to step 3 on the same model: the stamps of steps 4..6 are still in the slots' memory and must not be believed
    # when the sequence passes them again -- the two steps repeat their losses bit for bit (the second one's depends on
    # what the first one's apply wrote)
    m.restore(None, prefix)
    m.clip = 0.05
    for n, per in list(enumerate(_oracle_batches(cfg, world)))[3:5]:
        m.train_async(batch_tuple(per[rank]), lr)
        assert float(m.last_loss.item()) == losses[n], (n, float(m.last_loss.item()), losses[n])
    return out


def _oracle_case(rank, world, optimizer, reg, ckpt, reps):
    runs = []
    for rep in range(reps):
        losses, params, slots, m, cfg, cat, sq = _oracle_run(rank, world, optimizer, reg, os.path.join(ckpt, "rep%d" % rep))
        runs.append((losses, params, slots))
        # the running sums of squares after the six steps (this rank's rows; the category table), kept by the touched
        # rows' changes since the restore at step 3, against the tables themselves
        mine = [None] * world
        dist.all_gather_object(mine, sq[0])
        ref = sum(float((np.asarray(params[k], np.float64) ** 2).sum()) for k in ("item_emb", "user_emb", "usert_emb"))
        assert abs(sum(mine) - ref) <= 1e-6 * ref, (mine, ref)
        ref_c = float((np.asarray(params["cate_emb"], np.float64) ** 2).sum())
        assert abs(sq[1] - ref_c) <= 1e-6 * ref_c, (sq[1], ref_c)
    if reps == 1:
        # everything that only reads the parameters runs on such a model
        tb = random_batch(cfg, B=12, Sn=2, seed=790 + rank, test=True)[0]
        eb = (tb["u"], tb["i"], tb["j"], tb["hist_i"], tb["hist_i_new"], tb["hist_t"], tb["sl"], tb["sl_new"], tb["u_cate"])
        assert 0.0 <= m.eval_auc(None, eb) <= 1.0
        ids, sc = m.recommend(eb, 5)
        assert tuple(ids.shape) == (12, 5) and bool(torch.isfinite(sc).all())
        assert tuple(m.score_candidates(eb, np.stack([tb["i"], tb["j"]], 1)).shape) == (12, 2)
        r = m.label_ranks(eb).cpu().numpy()
        assert ((r >= 0) & (r < cfg["item_count"])).all()
    for losses, params, slots in runs[1:]:          # bitwise determinism
        assert losses == runs[0][0]
        for k in params:
            assert np.array_equal(params[k], runs[0][1][k]), k
            for j in range(2):
                assert np.array_equal(slots[j][k], runs[0][2][j][k]), k


@pytest.mark.parametrize("world,optimizer", [(2, "adam"), (2, "rmsprop"), (2, "adadelta"), (1, "adam")])
def test_sharded_lazy_optimizers_track_the_restricted_oracle(world, optimizer, tmp_path):
    """Tables much larger than a batch, non-zero slots everywhere: five clipped steps and one unclipped one.  Loss, used
    rows, dense weights and their slots follow the restricted oracle on the concatenated batch within the single-GPU
    test's bounds; rows no rank used keep W and both slots bit for bit; both checkpoint formats restore the state."""
    run_ranks(_oracle_case, world, optimizer, 1e-3, str(tmp_path), 1)


def test_sharded_lazy_adam_is_bitwise_reproducible(tmp_path):
    """The two-rank Adam run done twice: identical losses, parameters and slots."""
    run_ranks(_oracle_case, 2, "adam", 1e-3, str(tmp_path), 2)


def test_sharded_lazy_running_sums_of_squares(tmp_path):
    """regulation_rate = 0.05, where the L2 term carries the loss: the oracle parity of the six steps still holds, and
    the running sums (_sq) equal the sums of squares of the gathered tables to 1e-6 (checked in _oracle_case)."""
    run_ranks(_oracle_case, 2, "adam", 0.05, str(tmp_path), 1)


def _one_rank_categories(rank, world):
    cfg = make_config(U=300, I=450, C=64, d=64, regulation_rate=1e-3, max_gradient_norm=0.05, optimizer="lazy_adam")
    rng = np.random.RandomState(5)
    cat = rng.choice(np.arange(10), cfg["item_count"]).astype(np.int32)
    p = p32(random_params(cfg, seed=91))
    st = random_slots(p, "adam", 92)
    m = sharded(cfg, cat, p, [st["slot1"], st["slot2"]])
    names = ("cate_s1", "cate_s2")
    start = [m.cate_emb.cpu().numpy()] + [m.slots[k].cpu().numpy() for k in names]
    for s in range(2):
        b = random_batch(cfg, B=20, Sn=2, seed=900 + 10 * s + rank)[0]
        b["u_cate"] = rng.choice(np.arange(10, 15) if rank == 0 else np.arange(15, 18), 20).astype(np.int64)
        if s == 0:     # every category of the rank's range is named at least once
            own = np.arange(10, 15) if rank == 0 else np.arange(15, 18)
            b["u_cate"][:len(own)] = own
        m.train_async(batch_tuple(b), 0.05)
    end = [m.cate_emb.cpu().numpy()] + [m.slots[k].cpu().numpy() for k in names]
    for a, b0 in zip(end, start):
        assert np.array_equal(a[18:], b0[18:])                       # nobody's categories: bit for bit
        assert all((a[c] != b0[c]).any() for c in range(10, 18))     # one rank's u_cate: moved on both ranks
    mine = end + [m.dense.cpu().numpy(), m.slots["dense_s1"].cpu().numpy(), m.slots["dense_s2"].cpu().numpy()]
    every = [None] * world
    dist.all_gather_object(every, mine)
    for other in every:
        for a, b0 in zip(other, mine):
            assert np.array_equal(a, b0)


def test_sharded_lazy_categories_seen_by_one_rank_only():
    """Item categories 0..9, rank 0's u_cate 10..14, rank 1's 15..17, 64 categories: rows 18..63 of cate_emb and of both
    slots keep their bits, rows 10..17 move on BOTH ranks, and the replicated state is bitwise the same on both."""
    run_ranks(_one_rank_categories, 2)


def _equals_dense(rank, world):
    base = make_config(U=40, I=60, C=7, d=64, regulation_rate=1e-3, max_gradient_norm=0.05)
    _, cat = random_batch(base, B=8, Sn=3, seed=1)
    full = cover_all_batch(base, 740)
    B = len(full["u"])
    mine = {k: v[rank * B // world:(rank + 1) * B // world] for k, v in full.items()}
    for optimizer in ("adam", "rmsprop", "adadelta"):
        p = p32(random_params(base, seed=73))
        st = random_slots(p, optimizer, 74)
        out = []
        for name, l2 in ((optimizer, "dense"), ("lazy_" + optimizer, "lazy")):
            m = sharded(dict(base, optimizer=name), cat, p, [st["slot1"], st["slot2"]], l2_mode=l2)
            m.train_async(batch_tuple(mine), LR[optimizer])
            out.append((float(m.last_loss.item()), m.gather_params(), m.gather_slots()))
        (ld, pd, sd), (ll, pl, sl) = out
        assert abs(ld - ll) <= 1e-6 * max(1.0, abs(ld)), (optimizer, ld, ll)
        for k in pd:
            scale = np.abs(pd[k] - np.asarray(p[k], np.float32).reshape(pd[k].shape)).max() + 1e-30
            assert np.abs(pl[k] - pd[k]).max() <= 1e-5 * scale + 1e-7, (optimizer, k)
            for j in range(2):
                assert np.abs(sl[j][k] - sd[j][k]).max() <= 1e-5 * np.abs(sd[j][k]).max() + 1e-12, (optimizer, k)


def test_sharded_lazy_equals_sharded_dense_when_every_row_is_used():
    """One global batch that uses every row of every table, split over two ranks: sharded lazy_X and sharded X from the
    same parameters and slots agree to fp32 rounding."""
    run_ranks(_equals_dense, 2)


def test_sharded_train_driver_with_lazy_adam(tmp_path):
    """python -m tlsan_amd.train --sharded 1 --optimizer lazy_adam over two ranks against the single-GPU driver with
    the same flags (40 steps, batch 33, the bounds of test_sharded_train_driver_matches_single_gpu)."""
    extra = ("--optimizer", "lazy_adam", "--learning_rate", "0.01")
    run_ranks(driver_worker, 2, str(tmp_path), extra)


# (di, Ls, dc, ranks): the four row-width forms of the kernel (64 NCH floats per row, NCH = 1..4), and more ranks than it
# keeps sources in flight (four up to 128 columns, two beyond), so that the source loop runs more than once
APPLY_CASES = [("adam", 32, 10, 32, 1), ("rmsprop", 64, 10, 64, 3), ("adadelta", 64, 10, 64, 6), ("adam", 128, 10, 128, 3),
               ("rmsprop", 128, 90, 128, 5)]


@pytest.mark.parametrize("kind,di,Ls,dc,G", APPLY_CASES)
def test_apply_lazy_opt_against_numpy(kind, di, Ls, dc, G):
    """tlsan_shard_apply_lazy_opt on made-up received rows against numpy in float64: rows several sources send (summed in
    source order), rows one source sends, item rows whose item_b gradient is exactly zero, NaN in the gradient rows'
    padding, used and unused categories.  Bounds: fp32 rounding of a handful of operations per element -- 1e-5 of the
    largest move for W, 1e-5 relative for the slots; everything not used keeps its bits; the sums of squares move by the
    written rows' change; two calls on the same input leave the same bits."""
    import ctypes as C
    from tlsan_amd import _lib as L
    from tlsan_amd.model import OPTIMIZERS
    lib = L.load()
    code, b1, b2, eps = OPTIMIZERS[kind]
    rng = np.random.RandomState(di + Ls + G)
    W = max(di + 4, (di + Ls + 3) // 4 * 4)
    cI, R, Cn, step, lr, coef, reg, stamp = 150, 330, 37, 3, 0.05, 0.37, 1e-2, 77
    per = [np.sort(rng.choice(R, rng.randint(20, 60), replace=False)).astype(np.int32) for _ in range(G)]
    if G > 1:
        per[-1] = np.unique(np.concatenate([per[-1], per[0][:7]])).astype(np.int32)     # rows the first and the last send
    rows = np.concatenate(per)
    src_off = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int32)
    n_recv = len(rows)
    vals = rng.randn(n_recv, W).astype(np.float32)
    live = np.where(rows < cI, di + 1, di + Ls)
    vals[np.arange(W)[None, :] >= live[:, None]] = np.nan                            # never looked at
    quiet = np.unique(rows[rows < cI])[::3]                                          # items that only histories use
    vals[np.isin(rows, quiet), di] = 0.0
    shard0 = rng.uniform(-0.8, 0.8, (R, W)).astype(np.float32)
    cate0 = rng.uniform(-0.8, 0.8, (Cn, dc)).astype(np.float32)
    g_cate = rng.randn(Cn, dc).astype(np.float32)
    use = ((rng.rand(Cn) < 0.5) * rng.randint(1, G + 1, Cn)).astype(np.float32)    # the number of ranks that used it
    sl0 = {k: rng.uniform(1e-3, 2e-3, sh).astype(np.float32)
           for k, sh in (("shard_s1", (R, W)), ("shard_s2", (R, W)), ("cate_s1", (Cn, dc)), ("cate_s2", (Cn, dc)))}
    # ---- numpy
    ref_w, ref_c = shard0.astype(np.float64), cate0.astype(np.float64)
    ref = {k: v.astype(np.float64) for k, v in sl0.items()}
    acc = np.zeros((R, W))
    got_any = np.zeros(R, bool)
    for e, r in enumerate(rows):                                                     # (concatenated in source order)
        acc[r] += np.nan_to_num(vals[e].astype(np.float64))
        got_any[r] = True
    moved = np.zeros((R, W), bool)
    for r in np.nonzero(got_any)[0]:
        nreg = di if r < cI else di + Ls
        g = acc[r] / G
        g[:nreg] += reg * ref_w[r, :nreg]
        cols = np.arange(W) < nreg
        if r < cI and g[di] != 0.0:
            cols[di] = True
        moved[r] = cols
        ref_w[r, cols], ref["shard_s1"][r, cols], ref["shard_s2"][r, cols] = _np_opt_elem(
            kind, lr, b1, b2, eps, step, ref_w[r, cols], coef * g[cols], ref["shard_s1"][r, cols], ref["shard_s2"][r, cols])
    cu = use != 0
    gc = g_cate[cu].astype(np.float64) / G + reg * ref_c[cu]
    ref_c[cu], ref["cate_s1"][cu], ref["cate_s2"][cu] = _np_opt_elem(kind, lr, b1, b2, eps, step, ref_c[cu], coef * gc,
                                                                    ref["cate_s1"][cu], ref["cate_s2"][cu])
    assert moved.any(1).sum() < R and 0 < cu.sum() < Cn and (moved[quiet, di] == False).all() and moved[:cI, di].any()
    # ---- device
    dev = lambda a: torch.as_tensor(a).cuda()
    outs = []
    for rep in range(2):
        shard, cate = dev(shard0), dev(cate0)
        sl = {k: dev(v) for k, v in sl0.items()}
        opt = L.ShardOptimizer(code | L.OPT_LAZY, step, b1, b2, eps, sl["shard_s1"].data_ptr(), sl["shard_s2"].data_ptr(),
                               sl["cate_s1"].data_ptr(), sl["cate_s2"].data_ptr(), None, None, None)
        slots64 = torch.zeros(R * G, dtype=torch.int64, device="cuda")
        sq = torch.tensor([5.0, 7.0], dtype=torch.float64, device="cuda")
        sq32 = torch.zeros(1, device="cuda")
        step_dev = dev(np.array([lr * coef, coef, 0, 0], np.float32))
        nws = int(lib.tlsan_shard_apply_lazy_opt_workspace(n_recv, Cn))
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        keep = [dev(x) for x in (vals, rows, g_cate, use)]
        L.check(lib.tlsan_shard_apply_lazy_opt(shard.data_ptr(), W, cI, R, W, di, di + Ls, keep[0].data_ptr(), W, keep[1].data_ptr(),
                                               n_recv, (C.c_int32 * (G + 1))(*src_off.tolist()), G, slots64.data_ptr(), stamp,
                                               1.0 / G, step_dev.data_ptr(), reg, cate.data_ptr(), Cn, dc, keep[2].data_ptr(),
                                               keep[3].data_ptr(), sq.data_ptr(), sq32.data_ptr(), C.byref(opt), lr,
                                               ws.data_ptr(), nws, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "tlsan_shard_apply_lazy_opt")
        outs.append([t.cpu().numpy() for t in (shard, cate, sl["shard_s1"], sl["shard_s2"], sl["cate_s1"], sl["cate_s2"], sq, sq32)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    shard, cate, s1, s2, c1, c2, sq, sq32 = outs[0]
    for got, want, start, mask in ((shard, ref_w, shard0, moved), (cate, ref_c, cate0, cu[:, None] & np.ones_like(cate0, bool))):
        assert np.array_equal(got[~mask], start[~mask])
        assert np.abs(got - want)[mask].max() <= 1e-5 * np.abs(want - start).max() + 1e-7
    for got, want, start, mask in ((s1, ref["shard_s1"], sl0["shard_s1"], moved), (s2, ref["shard_s2"], sl0["shard_s2"], moved),
                                   (c1, ref["cate_s1"], sl0["cate_s1"], cu), (c2, ref["cate_s2"], sl0["cate_s2"], cu)):
        assert np.array_equal(got[~mask], start[~mask])
        assert np.abs(got - want)[mask].max() <= 1e-5 * np.abs(want[mask]).max() + 1e-12
    regm = np.arange(W)[None, :] < np.where(np.arange(R) < cI, di, di + Ls)[:, None]
    d0 = (shard.astype(np.float64) ** 2 - shard0.astype(np.float64) ** 2)[regm].sum()
    d1 = (cate.astype(np.float64) ** 2 - cate0.astype(np.float64) ** 2).sum()
    assert abs(sq[0] - (5.0 + d0)) <= 1e-9 * max(1.0, abs(d0)) and abs(sq[1] - (7.0 + d1)) <= 1e-9 * max(1.0, abs(d1))
    assert sq32[0] == np.float32(sq[0])


def test_cate_use_flags_match_numpy():
    """tlsan_shard_cate_use: 1 for the categories of the compact table's item rows (-1: no item) and of u_cate, 0 for
    the rest, whatever the buffer held; more than one workgroup, ids outside the table ignored."""
    import ctypes as C
    from tlsan_amd import _lib as L
    lib = L.load()
    rng = np.random.RandomState(8)
    Cn, n, B = 1000, 700, 37
    cate_c = rng.randint(-1, 300, n).astype(np.int32)
    cate_c[5] = Cn          # (never produced by the plan; must not be written)
    u_cate = rng.randint(600, 650, B).astype(np.int32)
    use = torch.full((Cn + 1,), 7.0, device="cuda")
    cc, uc = torch.as_tensor(cate_c).cuda(), torch.as_tensor(u_cate).cuda()
    L.check(lib.tlsan_shard_cate_use(cc.data_ptr(), n, uc.data_ptr(), B, Cn, use.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tlsan_shard_cate_use")
    ref = np.zeros(Cn + 1, np.float32)
    ref[cate_c[(cate_c >= 0) & (cate_c < Cn)]] = 1.0
    ref[u_cate] = 1.0
    ref[Cn] = 7.0           # past the C flags: untouched
    assert np.array_equal(use.cpu().numpy(), ref)
    assert 0 < ref[:Cn].sum() < Cn


def _refusals(rank, world):
    from tlsan_amd.dist import ShardedModel
    cfg = make_config(U=40, I=60, C=7, d=64, optimizer="lazy_adam")
    _, cat = random_batch(cfg, B=8, Sn=3, seed=1)
    for kw in (dict(l2_mode="lazy", static_rows=True), dict(l2_mode="lazy", static_rows=64, wire_dtype="bf16"), dict()):
        with pytest.raises(NotImplementedError, match="lazy"):
            ShardedModel(cfg, cat, device="cuda:0", **kw)
    ShardedModel(cfg, cat, device="cuda:0", l2_mode="lazy")      # and this is the form that exists


def test_sharded_lazy_refusals():
    """The static-shape step (and with it graph capture and bf16 rows on the wire) has no lazy optimizer, and the default
    l2_mode has none either: NotImplementedError at construction."""
    run_ranks(_refusals, 1)

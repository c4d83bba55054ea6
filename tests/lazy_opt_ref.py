"""What the tests of the lazy optimizers share (tests/test_gpu_lazy_opt.py, test_gpu_adagrad.py, test_gpu_dist_lazy_opt.py,
tests/adagrad_ref.py, scripts/lazy_rows_digest.py): the restricted oracle -- the dense optimizer's step from the same
parameters and slots (oracle.tlsan_oracle.train_step), after which every row the batch did not use is put back, in W and
both slots -- the rows a batch uses, slots to start from, the comparison of a model with that reference, and the check of
the sharded training driver against the single-GPU one.  Importable without a GPU."""
import copy
import os

import numpy as np

from oracle import tlsan_oracle as orc
from tests.helpers import random_batch

ROW_TABLES = ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb")
LR = {"adam": 0.05, "rmsprop": 0.02, "adadelta": 1.0}


def used_rows(b, cat, cfg):
    """Boolean masks of the rows a batch uses, per table (the index's used-row records)."""
    U, I, Cn, Ls = cfg["user_count"], cfg["item_count"], cfg["cate_count"], cfg["Ls"]
    uu = np.zeros(U, bool)
    uu[b["u"]] = True
    ui = np.zeros(I, bool)
    ui[b["i"]] = True
    Sn = b["hist_i_new"].shape[1]
    ui[b["hist_i"][np.arange(Ls)[None, :] < b["sl"][:, None]]] = True
    if Sn:
        ui[b["hist_i_new"][np.arange(Sn)[None, :] < b["sl_new"][:, None]]] = True
    uc = np.zeros(Cn, bool)
    uc[np.asarray(cat)[ui]] = True
    uc[b["u_cate"]] = True
    ub = np.zeros(I, bool)
    ub[b["i"]] = True
    return {"user_emb": uu, "usert_emb": uu, "item_emb": ui, "item_b": ub, "cate_emb": uc}


def restricted_step(q, st, cat, b, cfg, lr, optimizer, clip):
    """The lazy step's reference: the dense oracle step, with every unused row of W and both slots put back."""
    q0, s0 = copy.deepcopy(q), copy.deepcopy(st)
    loss, newq, info = orc.train_step(q, cat, b, cfg["num_heads"], cfg["regulation_rate"], lr=lr, clip=clip,
                                      optimizer=optimizer, opt_state=st)
    used = used_rows(b, cat, cfg)
    # item_b moves where its fp32 gradient is non-zero: a candidate whose sigmoid saturates to exactly its label in fp32
    # has gradient 0 there (and keeps its slots, as under the dense RMSProp / Adadelta) while the fp64 oracle still sees a
    # tiny one -- such rows are compared nowhere (`amb`: every use of the item as a candidate near saturation)
    near = np.abs(np.asarray(info["logits"], np.float64).reshape(-1)) > 15.0
    amb = np.zeros_like(used["item_b"])
    amb[np.asarray(b["i"])[near]] = True
    amb[np.asarray(b["i"])[~near]] = False
    used = dict(used, item_b_amb=amb)
    for k, mask in used.items():
        if k == "item_b_amb":
            continue
        newq[k] = np.where(mask.reshape((-1,) + (1,) * (q0[k].ndim - 1)), newq[k], q0[k])
        for s in ("slot1", "slot2"):
            st[s][k] = np.where(mask.reshape((-1,) + (1,) * (q0[k].ndim - 1)), st[s][k], s0[s][k])
    return loss, newq, info, used


def random_slots(p, optimizer, seed):
    """Non-zero slots on every row (a sweep over unused rows would show), valid for the optimizer (v, rms >= 0)."""
    rng = np.random.RandomState(seed)
    st = orc.init_opt_state(p, optimizer)
    for k in p:
        sh = np.shape(p[k])
        if optimizer == "adam":
            st["slot1"][k] = rng.uniform(-0.01, 0.01, sh)
            st["slot2"][k] = rng.uniform(1e-5, 1e-4, sh)
        elif optimizer == "rmsprop":
            st["slot1"][k] = rng.uniform(0.5, 1.5, sh)
            st["slot2"][k] = np.zeros(sh)                 # (momentum 0: the slot is recomputed, never decayed)
        else:
            st["slot1"][k] = rng.uniform(1e-5, 1e-3, sh)
            st["slot2"][k] = rng.uniform(1e-6, 1e-4, sh)
        for s in ("slot1", "slot2"):
            st[s][k] = np.asarray(st[s][k], np.float32).astype(np.float64)
    return st


def compared(k, a, used):
    """the rows of parameter k that are compared (item_b: not the saturated candidates, see restricted_step)"""
    a = np.asarray(a, np.float64)
    return a[~used["item_b_amb"]] if k == "item_b" else a


def sync_amb(m, q, st, used):
    """carry the device's item_b (and its slots) of the saturated candidates into the reference for the next steps"""
    amb = used["item_b_amb"]
    if amb.any():
        q["item_b"] = np.where(amb, np.asarray(m.item_b.cpu().numpy(), np.float64), q["item_b"])
        for j, s in enumerate(m.get_slots()):
            st["slot%d" % (j + 1)]["item_b"] = np.where(amb, np.asarray(s["item_b"], np.float64),
                                                        st["slot%d" % (j + 1)]["item_b"])


def check_step(m, q, st, p_prev, used, tol_n, skip_b2=True, exact_unused=None):
    got = m.get_params()
    s1, s2 = m.get_slots()
    for k in q:
        if skip_b2 and k.endswith("_b2"):
            continue      # (gradient = rounding noise, see test_gpu_parity.test_other_optimizers_track_oracle)
        a = compared(k, np.asarray(got[k], np.float64).reshape(np.shape(q[k])), used)
        r, r0 = compared(k, q[k], used), compared(k, p_prev[k], used)
        step = np.abs(r - r0).max()
        assert np.abs(a - r).max() < 2e-3 * step * tol_n + 1e-7, k
        for gs, ref in ((s1[k], st["slot1"][k]), (s2[k], st["slot2"][k])):
            gs, ref = compared(k, np.asarray(gs).reshape(np.shape(ref)), used), compared(k, ref, used)
            assert np.abs(gs - ref).max() < 2e-3 * np.abs(ref).max() + 1e-9, k
    if exact_unused is not None:
        P0, S0 = exact_unused
        for k in ROW_TABLES:
            keep = ~used[k]
            assert np.array_equal(np.asarray(got[k], np.float32)[keep], np.asarray(P0[k], np.float32)[keep]), k
            assert np.array_equal(np.asarray(s1[k], np.float32)[keep], np.asarray(S0[0][k], np.float32)[keep]), k
            assert np.array_equal(np.asarray(s2[k], np.float32)[keep], np.asarray(S0[1][k], np.float32)[keep]), k


def cover_all_batch(cfg, seed):
    """One batch whose candidates cover every item, users every user and u_cate every category."""
    I, U, Cn = cfg["item_count"], cfg["user_count"], cfg["cate_count"]
    B = max(I, U, Cn)
    b, _ = random_batch(cfg, B=B, Sn=2, seed=seed)
    rng = np.random.RandomState(seed + 1)
    b["i"] = rng.permutation(np.arange(B) % I).astype(np.int64)
    b["u"] = rng.permutation(np.arange(B) % U).astype(np.int64)
    b["u_cate"] = rng.permutation(np.arange(B) % Cn).astype(np.int64)
    return b


SPARSE_CATEGORY_CASES = [("adam", 400, range(0, 10), range(200, 400), 16, 64),       # one category per workgroup
                         ("adadelta", 1000, range(0, 20), range(500, 1000), 16, 128),  # wide rows
                         ("adam", 6, [0, 1], [2], 96, 64)]                              # shared categories (Rc64)


def driver_worker(rank, world, ckpt, extra):
    from tlsan_amd import train as T
    ds = os.path.join(os.path.dirname(__file__), "golden", "packed_clothing.npz")
    # batch 33 over 2 ranks: uneven shares (16 / 17) -> the weighted means; test batches of 128 split 64 / 64,
    # the last one (2010 % 128 = 90) 45 / 45
    argv = ["--dataset", ds, "--max_steps", "40", "--eval_freq", "20", "--quiet", "--train_batch_size", "33",
            "--model_dir", os.path.join(ckpt, "r%d" % rank), "--device_input", "0"] + list(extra)
    res = T.train_sharded(T.parse(argv + ["--sharded", "1"]))
    if rank == 0:
        one = T.train(T.parse(argv))
        assert res["steps"] == one["steps"] == 40 and res["world"] == world
        assert abs(res["init_auc"] - one["init_auc"]) < 1e-9, (res["init_auc"], one["init_auc"])
        assert abs(res["final_auc"] - one["final_auc"]) < 2e-3, (res["final_auc"], one["final_auc"])
        for a, b in zip(res["history"], one["history"]):
            assert a[0] == b[0] and abs(a[2] - b[2]) < 2e-3, (a, b)
        assert np.allclose(res["recall"], one["recall"], atol=2e-3), (res["recall"], one["recall"])
        assert np.allclose(res["prec"], one["prec"], atol=2e-3), (res["prec"], one["prec"])

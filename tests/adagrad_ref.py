"""The reference of lazy Adagrad and row-wise Adagrad (include/tlsan.h: TLSAN_OPT_ADAGRAD / TLSAN_OPT_ROWWISE_ADAGRAD with
TLSAN_OPT_LAZY) in numpy fp64: TF 1.8's ApplyAdagrad -- acc += g^2, w -= lr g / sqrt(acc), no epsilon -- on the clipped
gradients of the oracle, per element or with one accumulator per table row (acc_row += mean_j g_j^2), restricted to the rows
the batch used.  The rule functions need no GPU; restricted_adagrad_step needs the oracle only."""
import copy

import numpy as np

from oracle import tlsan_oracle as orc

ROW_KEYS = ("item_emb", "user_emb", "usert_emb", "cate_emb")     # the tables whose row-wise accumulator is [rows]
KINDS = ("lazy_adagrad", "lazy_rowwise_adagrad")
INITIAL_ACCUMULATOR = 0.1


def elementwise_rule(w, g, acc, lr):
    """-> (w', acc'): one accumulator per element"""
    w, g, acc = (np.asarray(x, np.float64) for x in (w, g, acc))
    acc = acc + g * g
    return w - lr * g / np.sqrt(acc), acc


def rowwise_rule(w, g, acc, lr):
    """w, g: [rows, n]; acc: [rows] -> (w', acc'): the row's accumulator takes the mean of the row's squared gradients, and
    every column steps with the new value"""
    w, g, acc = (np.asarray(x, np.float64) for x in (w, g, acc))
    acc = acc + (g * g).mean(axis=1)
    return w - lr * g / np.sqrt(acc)[:, None], acc


def is_row_slot(kind, k):
    return kind == "lazy_rowwise_adagrad" and k in ROW_KEYS


def random_accumulators(p, kind, seed):
    """uniform(0.05, 0.5) rounded to fp32 on EVERY row (a sweep over unused rows would show)"""
    rng = np.random.RandomState(seed)
    return {k: rng.uniform(0.05, 0.5, np.shape(v)[:1] if is_row_slot(kind, k) else np.shape(v)).astype(np.float32).astype(np.float64)
            for k, v in p.items()}


def initial_accumulators(p, kind):
    return {k: np.full(np.shape(v)[:1] if is_row_slot(kind, k) else np.shape(v), np.float64(np.float32(INITIAL_ACCUMULATOR)))
            for k, v in p.items()}


def restricted_adagrad_step(q, acc, cat, b, cfg, lr, kind, clip):
    """One lazy step from parameters q and accumulators acc (dicts of fp64 arrays; acc is updated in place).
    -> (loss, new parameters, info, used): info carries the oracle's and "g", the clipped gradients; used the row masks of
    tests/lazy_opt_ref.py's used_rows with its saturated-candidate entry item_b_amb."""
    from tests.lazy_opt_ref import used_rows
    assert kind in KINDS
    q = {k: np.asarray(v, np.float64) for k, v in q.items()}
    loss, _, info = orc.train_step(q, cat, b, cfg["num_heads"], cfg["regulation_rate"], lr=lr, clip=clip, optimizer="sgd")
    g = {k: info["coef"] * np.asarray(info["grads"][k], np.float64) for k in q}     # (the tables' already hold reg * W)
    acc0 = copy.deepcopy(acc)
    newq = {}
    for k in q:
        if is_row_slot(kind, k):
            newq[k], acc[k] = rowwise_rule(q[k], g[k], acc[k], lr)
        else:
            newq[k], acc[k] = elementwise_rule(q[k], g[k], acc[k], lr)
    used = used_rows(b, cat, cfg)
    # (item_b: the saturated candidates are compared nowhere -- restricted_step of tests/lazy_opt_ref.py)
    near = np.abs(np.asarray(info["logits"], np.float64).reshape(-1)) > 15.0
    amb = np.zeros_like(used["item_b"])
    amb[np.asarray(b["i"])[near]] = True
    amb[np.asarray(b["i"])[~near]] = False
    used = dict(used, item_b_amb=amb)
    for k, mask in used.items():
        if k == "item_b_amb":
            continue
        newq[k] = np.where(mask.reshape((-1,) + (1,) * (q[k].ndim - 1)), newq[k], q[k])
        acc[k] = np.where(mask.reshape((-1,) + (1,) * (acc0[k].ndim - 1)), acc[k], acc0[k])
    return loss, newq, dict(info, g=g), used

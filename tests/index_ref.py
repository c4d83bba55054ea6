"""A batch's destination index in numpy, product by product, from the definitions in include/tlsan.h,
csrc/tlsan_index_args.h and csrc/tlsan_index.h -- the reference of tests/test_gpu_index.py, itself checked against a
brute-force construction by tests/test_index_ref_cpu.py.  Integer work and a fixed function of the batch's ids and lengths:
every product is exact.  No GPU, no torch.

A batch is the dict of tests/helpers.random_batch (u, i, hist_i [B, Ls], hist_i_new [B, Sn], sl, sl_new, u_cate)."""
import numpy as np

BAL_TAIL_KEY = 10     # the largest ranking key of a sample with a session of one entry or none (BalArgs, by_window == 0)
BAL_KEYS = 192        # ranking keys are clamped below this


def uses(batch, Ls, item_cate=None, cseg=False):
    """The destination rows a batch uses, one entry per use: dict(item=, user=, cate=) of int64 id arrays.
    Items: the window slots below min(sl, Ls), the session slots below min(sl_new, Sn) and the candidate i (padding is no
    use).  Users: u.  Categories: u_cate -- plus, with category segments (cseg), item_cate[id] of every item use."""
    hist_i = np.asarray(batch["hist_i"], np.int64)
    B = hist_i.shape[0]
    hist_n = np.asarray(batch["hist_i_new"], np.int64).reshape(B, -1)
    Sn = hist_n.shape[1]
    assert hist_i.shape == (B, Ls)
    sl = np.minimum(np.asarray(batch["sl"], np.int64), Ls)
    sn = np.minimum(np.asarray(batch["sl_new"], np.int64), Sn)
    item = np.concatenate([hist_i[np.arange(Ls)[None, :] < sl[:, None]],
                           hist_n[np.arange(Sn)[None, :] < sn[:, None]],
                           np.asarray(batch["i"], np.int64)])
    cate = np.asarray(batch["u_cate"], np.int64)
    if cseg:
        cate = np.concatenate([cate, np.asarray(item_cate, np.int64)[item]])
    return dict(item=item, user=np.asarray(batch["u"], np.int64), cate=cate)


def table(ids, n):
    """One table's side of the index: counts [n]; off [n + 1], the exclusive prefix of the counts with off[n] = all uses
    (cur == off[:n]); the records (id, first, count, 0) of the used rows, ascending by id; their number."""
    cnt = np.bincount(ids, minlength=n).astype(np.int64)
    assert cnt.shape == (n,)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    used = np.flatnonzero(cnt)
    rec = np.stack([used, off[used], cnt[used], np.zeros_like(used)], 1).reshape(-1, 4)
    return dict(cnt=cnt, off=off, rec=rec, n_uniq=len(used))


def hot_slots(rec, ap_hot):
    """Record slots of the rows with more than ap_hot uses (their number is n_hot; the list's order is the atomics')."""
    return set(np.flatnonzero(rec[:, 2] > ap_hot).tolist())


def rank_keys(sl, sl_new, Ls, Sn, by_window):
    """The cost a sample is ranked by: its window length when windows are streamed (by_window > 0); otherwise
    11 min(session, 15) + min(window, 10) for sessions of two or more entries, 10 - min(window, 10) below."""
    w = np.clip(np.minimum(np.asarray(sl, np.int64), Ls), 0, None)
    if by_window > 0:
        return np.minimum(w, BAL_KEYS - 1)
    s = np.clip(np.minimum(np.asarray(sl_new, np.int64), Sn), 0, 15)
    w = np.minimum(w, 10)
    return np.where(s >= 2, 11 * s + w, BAL_TAIL_KEY - w)


def ranking(sl, sl_new, Ls, Sn, by_window):
    """perm [16 G], G = ceil(B / 16): perm[16 g + j] = sample j of group g, B where there is none.
    The batch is ranked by key, descending and stable (ties in sample order).  The first H G ranks are dealt out in snake
    order, one sample per group and round, forwards on even rounds and backwards on odd ones: every round when keyed by
    window, else the rounds that hold the samples with sessions of two or more, H = min(16, ceil(n_heavy / G)).  The tail
    follows in contiguous runs of 16 - H per group.  by_window == 0 numbers the groups backwards."""
    B = len(sl)
    G = (B + 15) // 16
    key = rank_keys(sl, sl_new, Ls, Sn, by_window)
    order = np.argsort(-key, kind="stable")
    n_heavy = 16 * G if by_window > 0 else int((key > BAL_TAIL_KEY).sum())
    H = min(16, (n_heavy + G - 1) // G)
    rev = by_window == 0
    perm = np.full(16 * G, B, np.int64)
    for r, smp in enumerate(order):
        if r < H * G:
            j, idx = divmod(r, G)
            g, pos = (G - 1 - idx if j & 1 else idx), j
        else:
            g, k = divmod(r - H * G, 16 - H)
            pos = H + k
        perm[(G - 1 - g if rev else g) * 16 + pos] = smp
    return perm


def category_lists(u_cate, C):
    """The samples of every category, as sets (inside a category the list's order is the atomics')."""
    u_cate = np.asarray(u_cate, np.int64)
    return [set(np.flatnonzero(u_cate == c).tolist()) for c in range(C)]


def build(batch, U, I, C, Ls, item_cate=None, cseg=False, rank=False, by_window=0, ap_hot=48):
    """Every product of a batch's index: item / cate / user sides (table), hot (record slots of the hot item rows),
    perm (None when the batch is not ranked), lists (the samples of every category)."""
    us = uses(batch, Ls, item_cate, cseg)
    B = len(us["user"])
    Sn = np.asarray(batch["hist_i_new"]).reshape(B, -1).shape[1]
    ref = dict(item=table(us["item"], I), cate=table(us["cate"], C), user=table(us["user"], U))
    ref["hot"] = hot_slots(ref["item"]["rec"], ap_hot)
    ref["perm"] = ranking(batch["sl"], batch["sl_new"], Ls, Sn, by_window) if rank else None
    ref["lists"] = category_lists(batch["u_cate"], C)
    return ref

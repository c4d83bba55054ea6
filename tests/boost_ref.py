"""Numpy reference of the boosted lists (tlsan_eval_topk_scoped_boost / tlsan_eval_topk_lists_boost, recommend's boost= and
boost_weight=): the adjusted score in float32 with separate roundings,
    s' = fl(s + t),  t = boost[g] without row weights,  t = fl(weight[b] * boost[g]) with them,
and the selection on it in tf.nn.top_k's order -- higher s' first, equal s' (+0 == -0) -> lower id, NaN after everything
else, a zero returned as +0.0, short rows padded with -1 / -inf.  The raw scores are taken as they are (the model's own,
score_candidates'), so a boosted list can be compared with the kernel's bit for bit."""
import numpy as np


def adjusted(scores, boost, weight=None):
    """scores [B, n] float32 of the columns' items, boost [n] float32 of the same items, weight [B] float32 or None ->
    s' [B, n] float32: two float32 roundings with weights (the product, then the sum), one without."""
    s, b = np.asarray(scores), np.asarray(boost)
    assert s.dtype == np.float32 and b.dtype == np.float32 and b.shape == s.shape[1:]
    with np.errstate(all="ignore"):
        if weight is None:
            t = np.broadcast_to(b[None, :], s.shape)
        else:
            w = np.asarray(weight)
            assert w.dtype == np.float32 and w.shape == s.shape[:1]
            t = w[:, None] * b[None, :]                 # float32 * float32 -> float32: rounded once
            assert t.dtype == np.float32
        out = s + t
    assert out.dtype == np.float32
    return out


def order(adj, ids, ok):
    """The positions of one row's eligible columns in the list's order (ids: the columns' global ids)."""
    pos = np.nonzero(ok)[0]
    v = np.asarray(adj)[pos].astype(np.float64)
    nan = np.isnan(v)
    key = np.where(nan, 0.0, v) + 0.0
    return pos[np.lexsort((np.asarray(ids)[pos], -key, nan))]     # last key first: NaN flag, then s' descending, then id


def topk(adj, ids, k, excluded=None):
    """adj [B, n] float32 adjusted scores of the columns, ids [n] their global ids, excluded: None or [B, n] bool (True: the
    row may not select the column) -> (ids [B, k] int32, s' [B, k] float32)."""
    adj, ids = np.asarray(adj), np.asarray(ids, np.int64)
    assert adj.dtype == np.float32 and ids.shape == adj.shape[1:]
    B = adj.shape[0]
    ok = np.ones(adj.shape, bool) if excluded is None else ~np.broadcast_to(np.asarray(excluded, bool), adj.shape)
    out_ids = np.full((B, k), -1, np.int32)
    out_sc = np.full((B, k), -np.inf, np.float32)
    for r in range(B):
        o = order(adj[r], ids, ok[r])[:k]
        out_ids[r, :len(o)] = ids[o]
        out_sc[r, :len(o)] = adj[r, o] + np.float32(0.0)          # (-0.0 + 0.0 == +0.0)
    return out_ids, out_sc

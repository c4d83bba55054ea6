"""Numpy reference of the scoped lists (tlsan_eval_topk_scoped / tlsan_similar_topk_scoped, recommend's within= and
category=): the selection alone.  From a [B, I] score matrix and a mask of the eligible (row, item) pairs it gives the K
best eligible items of each row in tf.nn.top_k's order -- higher score first, equal scores (+0 == -0) -> lower id first,
a NaN score after every other score -- with a zero score returned as +0.0 and short rows padded with -1 / -inf.  The
scores are taken as they are (their dtype and bits are kept), so a list selected from the model's own scores can be
compared with the kernel's bit for bit."""
import numpy as np


def mask_of(B, I, within=None, category=None, item_cate=None, exclude=None):
    """[B, I] bool: item n is eligible for row b when it is in `within` (ids; None: all), its category is category[b]
    (negative: any; None: no test) and it is not in exclude[b] (B id collections; ids outside the table ignored)."""
    ok = np.ones((B, I), bool)
    if within is not None:
        inside = np.zeros(I, bool)
        inside[np.asarray(within, np.int64)] = True
        ok &= inside[None, :]
    if category is not None:
        category = np.asarray(category, np.int64)
        ok &= (category[:, None] < 0) | (np.asarray(item_cate, np.int64)[None, :] == category[:, None])
    if exclude is not None:
        for r, x in enumerate(exclude):
            x = np.asarray(sorted(x), np.int64).reshape(-1)
            ok[r, x[(x >= 0) & (x < I)]] = False
    return ok


def order(s, ok):
    """The eligible ids of one row in the list's order."""
    ids = np.nonzero(ok)[0]
    v = np.asarray(s)[ids].astype(np.float64)
    nan = np.isnan(v)
    key = np.where(nan, 0.0, v) + 0.0
    return ids[np.lexsort((ids, -key, nan))]     # last key first: NaN flag, then score descending, then id


def topk(scores, ok, K):
    """(ids [B, K] int32, scores [B, K] of scores' dtype)."""
    scores = np.asarray(scores)
    ok = np.broadcast_to(np.asarray(ok, bool), scores.shape)
    B = scores.shape[0]
    ids = np.full((B, K), -1, np.int32)
    sc = np.full((B, K), -np.inf, scores.dtype)
    for r in range(B):
        o = order(scores[r], ok[r])[:K]
        ids[r, :len(o)] = o
        sc[r, :len(o)] = scores[r, o] + scores.dtype.type(0.0)      # (-0.0 + 0.0 == +0.0)
    return ids, sc

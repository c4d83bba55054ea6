"""Numpy reference of the lists behind a cursor (tlsan_eval_topk_scoped_after / tlsan_eval_topk_lists_after /
tlsan_dense_topk_after, the after= of recommend and audience): a row's page is "the eligible columns strictly behind the
cursor, then tests/boost_ref.py's order".  Strictly behind (cs, cg) in that order -- higher score first, equal scores
(+0 == -0) -> lower id, NaN after everything else:
    cursor not NaN:  s is NaN,  or s < cs,  or s == cs and g > cg
    cursor NaN:      s is NaN and g > cg
A cursor id of START (-2) is no cursor, any other negative id an exhausted row (an empty page).  The scores are taken as
they are (the model's own, or boost_ref.adjusted's), so a page can be compared with the kernel's bit for bit."""
import numpy as np

from tests import boost_ref

START = -2


def behind(adj_row, ids, after_id, after_score):
    """[n] bool: the columns of one row (scores adj_row, global ids `ids`) strictly behind the cursor."""
    s, g = np.asarray(adj_row).astype(np.float64), np.asarray(ids, np.int64)
    if after_id == START:
        return np.ones(s.shape, bool)
    if after_id < 0:
        return np.zeros(s.shape, bool)
    nan = np.isnan(s)
    cs = float(after_score)
    if np.isnan(cs):
        return nan & (g > after_id)
    with np.errstate(invalid="ignore"):
        return nan | (s < cs) | ((s == cs) & (g > after_id))


def page(adj, ids, k, after_ids, after_scores, excluded=None):
    """adj [B, n] float32 scores of the columns, ids [n] their global ids, the rows' cursors [B], excluded None or [B, n]
    bool -> (ids [B, k] int32, scores [B, k] float32): the k best eligible columns behind each row's cursor."""
    adj, ids = np.asarray(adj), np.asarray(ids, np.int64)
    assert adj.dtype == np.float32 and ids.shape == adj.shape[1:]
    B = adj.shape[0]
    ok = np.ones(adj.shape, bool) if excluded is None else ~np.broadcast_to(np.asarray(excluded, bool), adj.shape)
    out_ids = np.full((B, k), -1, np.int32)
    out_sc = np.full((B, k), -np.inf, np.float32)
    for r in range(B):
        o = boost_ref.order(adj[r], ids, ok[r] & behind(adj[r], ids, int(after_ids[r]), after_scores[r]))[:k]
        out_ids[r, :len(o)] = ids[o]
        out_sc[r, :len(o)] = adj[r, o] + np.float32(0.0)          # (-0.0 + 0.0 == +0.0)
    return out_ids, out_sc


def cursor_of(page_ids, page_scores):
    """The cursor behind a page: its last column."""
    return np.array(page_ids[:, -1], np.int32), np.array(page_scores[:, -1], np.float32)


def start(B):
    return np.full(B, START, np.int32), np.zeros(B, np.float32)


def walk(adj, ids, k, pages, excluded=None, after=None):
    """`pages` pages of k chained through cursor_of from `after` (None: the start) -> the list of (ids, scores) pages."""
    after = start(np.asarray(adj).shape[0]) if after is None else after
    out = []
    for _ in range(pages):
        out.append(page(adj, ids, k, after[0], after[1], excluded))
        after = cursor_of(*out[-1])
    return out

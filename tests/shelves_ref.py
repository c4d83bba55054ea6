"""Numpy reference of the category shelves (tlsan_eval_shelves, Model.shelves): from a [B, I] score matrix (the model's own,
from score_candidates, so that bits can be compared), a mask of the eligible (row, item) pairs and the lists
(list_off, list_items) it gives each row's page -- the S lists whose own m-lists rank highest, with those m-lists.

L(b, c) is scope_ref.topk over the eligible items of list c (entries of the list outside [0, I) are no items); n(b, c) its
valid entries.  List c is a candidate of row b when skip[b] does not name it and n(b, c) >= min_items; its rank key is entry
rank_at of L(b, c).  Candidates are ordered by that entry in the lists' own order -- not NaN before NaN, higher score
first (+0 == -0), lower item id first -- and, for equal entries, by the lower list id."""
import numpy as np

from tests import scope_ref


def lists_of(scores, ok, list_off, list_items, m):
    """L(b, c) for every list: (ids [C, B, m] int32, scores [C, B, m])."""
    scores, ok = np.asarray(scores), np.asarray(ok, bool)
    B, I = scores.shape
    off, items = np.asarray(list_off, np.int64), np.asarray(list_items, np.int64)
    C = len(off) - 1
    ids = np.full((C, B, m), -1, np.int32)
    sc = np.full((C, B, m), -np.inf, scores.dtype)
    for c in range(C):
        held = items[off[c]:off[c + 1]]
        inside = np.zeros(I, bool)
        inside[held[(held >= 0) & (held < I)]] = True
        if inside.any():
            ids[c], sc[c] = scope_ref.topk(scores, ok & inside[None, :], m)
    return ids, sc


def page(lids, lsc, S, m, min_items=1, rank_at=0, skip=None):
    """The pages from lists_of's arrays (their first m entries are used) -> (cats [B, S] int32, ids [B, S, m] int32,
    scores [B, S, m]).  skip: None, [B] or [B, X] list ids (negative: nothing)."""
    C, B = lids.shape[:2]
    assert 1 <= min_items <= m <= lids.shape[2] and 0 <= rank_at < min_items
    lids, lsc = lids[:, :, :m], lsc[:, :, :m]
    if skip is not None:
        skip = np.asarray(skip, np.int64).reshape(B, -1)
    cats = np.full((B, S), -1, np.int32)
    ids = np.full((B, S, m), -1, np.int32)
    sc = np.full((B, S, m), -np.inf, lsc.dtype)
    for b in range(B):
        cand = []
        for c in range(C):
            if skip is not None and c in skip[b]:
                continue
            if (lids[c, b] >= 0).sum() < min_items:
                continue
            s = float(lsc[c, b, rank_at])
            nan = s != s
            cand.append((nan, 0.0 if nan else -(s + 0.0), int(lids[c, b, rank_at]), c))
        for j, (_, _, _, c) in enumerate(sorted(cand)[:S]):
            cats[b, j], ids[b, j], sc[b, j] = c, lids[c, b], lsc[c, b]
    return cats, ids, sc


def shelves(scores, ok, list_off, list_items, S, m, min_items=1, rank_at=0, skip=None):
    return page(*lists_of(scores, ok, list_off, list_items, m), S, m, min_items, rank_at, skip)

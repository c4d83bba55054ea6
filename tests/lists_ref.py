"""Numpy reference of the indexed lists (tlsan_eval_topk_lists / tlsan_similar_topk_lists, recommend's index=): which
(row, item) pairs are eligible.  Row b's candidates are the UNION of the lists row_lists[b, :] names -- a negative id or
one >= the number of lists is no probe, a repeated id counts once, an entry of a list outside [0, I) is not an item --
minus the row's exclusion list; the selection from them is tests/scope_ref.py's topk."""
import numpy as np


def index_of(item_cate, cate_count, within=None):
    """(list_off [C + 1], list_items) of a partition by category, ascending by (category, id); within: ids or None."""
    item_cate = np.asarray(item_cate, np.int64)
    ids = np.arange(len(item_cate)) if within is None else np.unique(np.asarray(within, np.int64))
    lists = [ids[item_cate[ids] == c] for c in range(cate_count)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, (np.concatenate(lists) if len(ids) else np.zeros(0, np.int64)).astype(np.int64)


def union_mask(B, I, row_lists, list_off, list_items, exclude=None):
    """[B, I] bool: item n is eligible for row b."""
    row_lists = np.asarray(row_lists, np.int64).reshape(B, -1)
    ok = np.zeros((B, I), bool)
    for b in range(B):
        for c in row_lists[b]:
            if 0 <= c < len(list_off) - 1:
                x = np.asarray(list_items[list_off[c]:list_off[c + 1]], np.int64)
                ok[b, x[(x >= 0) & (x < I)]] = True
        if exclude is not None:
            x = np.asarray(sorted(exclude[b]), np.int64).reshape(-1)
            ok[b, x[(x >= 0) & (x < I)]] = False
    return ok

"""Reference of the explanations (include/tlsan.h, tlsan_explain; Model.explain): the parts of a listed score in fp64 from
the oracle's forward, and the selection of the strongest sources from fp32 parts.  Test infrastructure: numpy only."""
import functools

import numpy as np

from oracle import tlsan_oracle as orc


def att_by_channel(att, B, H):
    """An attention tensor as [B, L, d]: from the kernels' [H * B, L, d / H] (row h * B + b) or the oracle's [B, L, H, d / H]."""
    att = np.asarray(att, np.float64)
    if att.ndim == 3:
        HB, L, dh = att.shape
        assert HB == H * B, (att.shape, H, B)
        att = att.reshape(H, B, L, dh).transpose(1, 2, 0, 3)
    assert att.shape[0] == B and att.shape[2] == H, att.shape
    return att.reshape(B, att.shape[1], -1)


def parts_ref(p, cat, b, H, items, att0=None, att1=None):
    """-> (parts, M), both [B, Kc, R] float64, R = 3 + Ls + Sn: the parts of score(b, items[b, k]) -- column 0 the bias, 1 the
    user part, 2 the bridge offset, 3 .. the long-term positions, 3 + Ls .. the session positions -- and per part the sum
    of the absolute values of its terms.  p: the true parameters (oracle names); att0 / att1: the attention weights to
    decompose under (the kernels' layout or the oracle's), None: the oracle's own.  Positions past sl / sl_new and items
    with a negative id are 0 in both."""
    cat = np.asarray(cat, np.int64)
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    items = np.asarray(items, np.int64)
    B, Kc = items.shape
    res = orc.forward(p, cat, b, H, want_cache=True)
    c = res["cache"]
    a0 = att_by_channel(res["att0"] if att0 is None else att0, B, H)      # [B, Ls, d]
    a1 = att_by_channel(res["att1"] if att1 is None else att1, B, H)      # [B, 1 + Sn, d]
    h, h_new, u_emb = c["h"], c["h_new"], c["u_emb"]
    Ls, Sn = h.shape[1], h_new.shape[1]
    g = np.maximum(items, 0)
    w = np.concatenate([p["item_emb"][g], p["cate_emb"][cat[g]]], -1)     # [B, Kc, d]
    K, k0 = p["dense_K"], p["dense_b"]
    parts = np.zeros((B, Kc, 3 + Ls + Sn))
    M = np.zeros_like(parts)
    parts[:, :, 0] = p["item_b"][g]
    M[:, :, 0] = np.abs(parts[:, :, 0])
    parts[:, :, 1] = np.einsum("bc,bkc->bk", u_emb, w)
    M[:, :, 1] = np.einsum("bc,bkc->bk", np.abs(u_emb), np.abs(w))
    x = a1[:, 0][:, None, :] * w                                           # a1[b, 0, :] o w_g
    parts[:, :, 2] = (x * k0).sum(-1)
    M[:, :, 2] = np.abs(x * k0).sum(-1)
    v = np.einsum("ij,bkj->bki", K, x)                                     # v_bg = K (a1[b, 0, :] o w_g)
    Mv = np.einsum("ij,bkj->bki", np.abs(K), np.abs(x))
    ah = a0 * h
    parts[:, :, 3:3 + Ls] = np.einsum("blc,bkc->bkl", ah, v)
    M[:, :, 3:3 + Ls] = np.einsum("blc,bkc->bkl", np.abs(ah), Mv)
    if Sn:
        an = a1[:, 1:] * h_new
        parts[:, :, 3 + Ls:] = np.einsum("bjc,bkc->bkj", an, w)
        M[:, :, 3 + Ls:] = np.einsum("bjc,bkc->bkj", np.abs(an), np.abs(w))
    keep = np.ones((B, 3 + Ls + Sn), bool)
    keep[:, 3:3 + Ls] = np.arange(Ls)[None, :] < np.asarray(b["sl"])[:, None]
    keep[:, 3 + Ls:] = np.arange(Sn)[None, :] < np.asarray(b["sl_new"])[:, None]
    keep = keep[:, None, :] & (items >= 0)[:, :, None]
    return np.where(keep, parts, 0.0), np.where(keep, M, 0.0)


def _before(va, pa, vb, pb, order):
    """source (va, column pa) comes before (vb, pb): NaN last, the larger key first, equal keys -> the lower column"""
    va, vb = float(va), float(vb)            # (exact: every float32 is a double)
    na, nb = va != va, vb != vb
    if na != nb:
        return nb
    if not na:
        ka, kb = (abs(va), abs(vb)) if order == "abs" else (va, vb)
        if ka != kb:
            return ka > kb
    return pa < pb


def select_ref(parts_f32, batch, items, r, by, order):
    """The r strongest history sources of every (row, item) from the fp32 parts [B, Kc, R] -> (src, item, value), each
    [B, Kc, r] (int32, int32, float32).  by "position": every valid position is a source; "item": the valid positions of a
    row with the same item id are one, valued at the sequential float32 sum of their parts in ascending column order, its
    src the lowest column.  order "positive" / "abs".  Fewer than r sources, and padding items: -1, -1, 0."""
    parts = np.asarray(parts_f32)
    assert parts.dtype == np.float32 and by in ("item", "position") and order in ("positive", "abs")
    items = np.asarray(items)
    B, Kc, R = parts.shape
    hist_i, hist_n = np.asarray(batch["hist_i"]), np.asarray(batch["hist_i_new"]).reshape(B, -1)
    Ls = hist_i.shape[1]
    src = np.full((B, Kc, r), -1, np.int32)
    item = np.full((B, Kc, r), -1, np.int32)
    val = np.zeros((B, Kc, r), np.float32)
    for bi in range(B):
        pos = [(3 + l, int(hist_i[bi, l])) for l in range(int(batch["sl"][bi]))] + \
              [(3 + Ls + j, int(hist_n[bi, j])) for j in range(int(batch["sl_new"][bi]))]
        if by == "item":
            groups = {}
            for col, g in pos:                       # (ascending columns)
                groups.setdefault(g, []).append(col)
            sources = [(cols[0], g, cols) for g, cols in groups.items()]
        else:
            sources = [(col, g, [col]) for col, g in pos]
        for k in range(Kc):
            if items[bi, k] < 0:
                continue
            cand = []
            for col, g, cols in sources:
                s = parts[bi, k, cols[0]]
                for cc in cols[1:]:
                    s = np.float32(s + parts[bi, k, cc])
                cand.append((np.float32(s), col, g))
            cand.sort(key=functools.cmp_to_key(lambda x, y: -1 if _before(x[0], x[1], y[0], y[1], order) else 1))
            for n, best in enumerate(cand[:r]):
                val[bi, k, n], src[bi, k, n], item[bi, k, n] = best
    return src, item, val

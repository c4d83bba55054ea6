"""Numpy reference of the similar-items lists (tlsan_similar_topk, Model.similar_items), in fp64 on the stored fp32
values: the scores of both metrics, the eligibility rule, the order (ties, +-0, NaN), and the check of a returned list
against them."""
import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32


def item_matrix(item_emb, cate_emb, item_cate):
    """w = [item_emb || cate_emb[item_cate]] as stored (float32 values), in fp64."""
    return np.concatenate([np.asarray(item_emb, np.float32), np.asarray(cate_emb, np.float32)[np.asarray(item_cate)]],
                          1).astype(np.float64)


def scores(w, qids, metric, P=1.0):
    """[Q, I] fp64 scores of the queries against every item.  dot: P^2 w_q . w_n; cosine: w_q . w_n / (|w_q| |w_n|), 0
    where a norm is 0 (inv = 0)."""
    wq = w[np.asarray(qids)]
    acc = wq @ w.T
    if metric == "dot":
        return acc * (float(P) * float(P))
    nrm = np.sqrt((w * w).sum(1))
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    return acc * inv[np.asarray(qids)][:, None] * inv[None, :]


def tolerance(w, qids, metric, P=1.0):
    """[Q, I] the first-order fp32 bound on a score's error, doubled.  dot: (D + 4) 2u P^2 sum_k |w_q[k] w_n[k]|;
    cosine: (2 D + 8) 2u (the normalised terms sum to at most 1; each norm carries about (D / 2 + 2) u)."""
    D = w.shape[1]
    if metric == "dot":
        return (D + 4) * 2 * U * float(P) ** 2 * (np.abs(w[np.asarray(qids)]) @ np.abs(w).T)
    return np.full((len(qids), w.shape[0]), (2 * D + 8) * 2 * U)


def eligible(n_items, qids, exclude=None):
    """[Q, I] bool: every item but the query itself and the row's excluded ids (repeats and foreign ids ignored)."""
    ok = np.ones((len(qids), n_items), bool)
    ok[np.arange(len(qids)), np.asarray(qids)] = False
    if exclude is not None:
        for r, x in enumerate(exclude):
            x = np.asarray(x, np.int64).reshape(-1)
            ok[r, x[(x >= 0) & (x < n_items)]] = False
    return ok


def order(s, ok):
    """The eligible ids of one row in the list's order: higher score first, equal scores (+0 == -0) -> lower id first,
    NaN after every other score."""
    ids = np.nonzero(ok)[0]
    v = np.asarray(s, np.float64)[ids]
    nan = np.isnan(v)
    key = np.where(nan, 0.0, v) + 0.0            # (-0.0 + 0.0 == +0.0: the zeros compare equal anyway)
    return ids[np.lexsort((ids, -key, nan))]     # last key first: NaN flag, then score descending, then id


def topk(s, ok, k):
    """(ids [Q, k], scores [Q, k]) of the reference: rows with fewer than k eligible items end in -1 / -inf; a zero score
    is +0.0."""
    Q = s.shape[0]
    ids = np.full((Q, k), -1, np.int64)
    sc = np.full((Q, k), -np.inf)
    for r in range(Q):
        o = order(s[r], ok[r])[:k]
        ids[r, :len(o)] = o
        sc[r, :len(o)] = s[r, o] + 0.0
    return ids, sc


def check_lists(ids, sc, s, ok, tol):
    """A returned (ids, sc) [Q, k] against reference scores s, eligibility ok and bound tol [Q, I]:
      the ids are distinct and eligible, the padding (-1 / -inf) comes last and only when the eligible items ran out;
      each returned score is within tol of the reference score of its id;
      returned scores are non-increasing, equal bits in ascending id;
      no eligible item left out has a reference score above the k-th returned one's by more than 2 tol."""
    ids, sc = np.asarray(ids), np.asarray(sc)
    Q, k = ids.shape
    assert sc.dtype == np.float32 and sc.shape == ids.shape
    for r in range(Q):
        n_ok = int(ok[r].sum())
        n = min(k, n_ok)
        got, gs = ids[r, :n].astype(np.int64), sc[r, :n]
        assert np.all(ids[r, n:] == -1) and np.all(sc[r, n:] == -np.inf), (r, ids[r], sc[r])
        assert np.all(got >= 0) and len(set(got.tolist())) == n, (r, got)
        assert np.all(ok[r, got]), (r, got[~ok[r, got]])
        err = np.abs(gs.astype(np.float64) - s[r, got])
        assert np.all(err <= tol[r, got]), (r, float((err - tol[r, got]).max()), float(err.max()))
        assert not np.any(np.signbit(gs[gs == 0])), r
        a, b = gs[:-1], gs[1:]
        assert np.all((a > b) | ((a == b) & (got[:-1] < got[1:]))), (r, gs, got)
        if n_ok > k:
            out = ok[r].copy()
            out[got] = False
            rest = np.nonzero(out)[0]
            assert np.all(s[r, rest] <= float(gs[-1]) + 2 * tol[r, rest]), (r, float((s[r, rest] - gs[-1]).max()))

"""Numpy reference of the audience lists (tlsan_dense_topk, Model.audience): the expected list from a given score matrix
-- score descending, NaN last, +0 == -0, then row ascending, minus the excluded rows, -1 / -inf padding -- and the
brute-force item -> rows exclusion from a seen-items CSR and a row -> user array."""
import numpy as np

from tests.similar_ref import order


def expected(scores, k, exclude=None, id_add=0):
    """scores [Q, N] (query q against matrix row n; float32 keeps its bits) -> (rows [Q, k] int32 of GLOBAL numbers id_add + n,
    scores [Q, k] of scores' dtype).  exclude: None or Q sequences of global row numbers (numbers outside the matrix match
    nothing).  A zero score comes back as +0.0."""
    scores = np.asarray(scores)
    Q, N = scores.shape
    rows = np.full((Q, k), -1, np.int32)
    out = np.full((Q, k), -np.inf, scores.dtype)
    for q in range(Q):
        ok = np.ones(N, bool)
        if exclude is not None:
            x = np.asarray(exclude[q], np.int64).reshape(-1) - id_add
            ok[x[(x >= 0) & (x < N)]] = False
        o = order(scores[q], ok)[:k]
        rows[q, :len(o)] = o + id_add
        out[q, :len(o)] = scores[q, o] + scores.dtype.type(0.0)
    return rows, out


def seen_rows(seen_off, seen_ids, user, items, row0=0):
    """Brute force: for each query item, the ascending global numbers row0 + n of the rows n whose user user[n] has the
    item in seen_ids[seen_off[u] : seen_off[u + 1]] (a user outside the CSR has seen nothing)."""
    seen_off, seen_ids, user = np.asarray(seen_off), np.asarray(seen_ids), np.asarray(user)
    n_users = len(seen_off) - 1
    out = []
    for it in np.asarray(items).tolist():
        out.append([row0 + n for n, u in enumerate(user.tolist())
                    if 0 <= u < n_users and it in seen_ids[seen_off[u]:seen_off[u + 1]].tolist()])
    return out


def brute_force(scores, k, exclude=None, id_add=0):
    """expected() by python loops and a comparison function, for checking the reference itself."""
    import functools
    scores = np.asarray(scores)
    Q, N = scores.shape

    def before(a, b):                      # (score, row): negative when a comes first
        (sa, ra), (sb, rb) = a, b
        na, nb = sa != sa, sb != sb
        if na != nb:
            return 1 if na else -1
        if not na and sa != sb:            # (+0.0 == -0.0 compares equal)
            return -1 if sa > sb else 1
        return -1 if ra < rb else (1 if ra > rb else 0)

    rows = np.full((Q, k), -1, np.int32)
    out = np.full((Q, k), -np.inf, scores.dtype)
    for q in range(Q):
        gone = set() if exclude is None else set(int(x) for x in exclude[q])
        cand = [(float(scores[q, n]), n + id_add) for n in range(N) if n + id_add not in gone]
        cand.sort(key=functools.cmp_to_key(before))
        for j, (s, r) in enumerate(cand[:k]):
            rows[q, j] = r
            out[q, j] = 0.0 if s == 0 else s
    return rows, out

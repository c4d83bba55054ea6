"""Numpy reference of the diversified lists (tlsan_rerank, recommend's diversity / per_category), in fp64 on the fp32
inputs: the greedy selection of one row, and the teacher-forced check of a returned selection -- a near-tie may flip a
greedy pick between fp32 and fp64, after which the two lists need not meet again, so a returned list is replayed step by
step with ITS OWN history and each pick is compared with the best value that history allowed.

One row's pool: ids [N] (global ids, -1 = padding), s [N] float32 scores in tlsan_eval_topk's order, w [N, d] stored
vectors, inv [N] inverse norms as given, cate [N].  theta in [0, 1], m >= 0 (0: no cap)."""
import numpy as np

U = 2.0 ** -24      # unit roundoff of fp32


def tau(d):
    """The bound on a pick's regret: 8 d 2^-24.  A value is (1 - theta) r - theta cos with r, cos in [-1, 1]: the d-term
    fp32 dot carries at most about (d / 16 + 4) u relative to |w_i| |w_j| (16 chains of d / 16 FMAs and a 4-level tree),
    the product of the two inverse norms and the scaling 3 u, the relevance (a difference, a quotient, a product) 3 u
    and the mix 2 u; both compared values carry it.  2 (d / 16 + 12) u <= 8 d u for every d >= 4."""
    return 8.0 * d * U


def valid(ids, s):
    return (np.asarray(ids) >= 0) & np.isfinite(np.asarray(s, np.float64))


def relevance(ids, s):
    """r_j = (s_j - s_lo) / (s_hi - s_lo) over the first / last valid entry's score; 0 when equal or without a valid entry."""
    s = np.asarray(s, np.float64)
    ok = valid(ids, s)
    r = np.zeros(len(s))
    pos = np.nonzero(ok)[0]
    if len(pos) and s[pos[0]] != s[pos[-1]]:
        hi, lo = s[pos[0]], s[pos[-1]]
        r[ok] = (s[ok] - lo) / (hi - lo)
    return r


class _Row:
    """The state of one row's greedy loop: eligibility and the values of a step, given the picks made so far."""

    def __init__(self, ids, s, w, inv, cate, theta, m):
        self.ok = valid(ids, s)
        self.r = relevance(ids, s)
        self.w = np.asarray(w, np.float64)
        self.inv = np.asarray(inv, np.float64)
        self.cate = np.asarray(cate)
        self.theta, self.m = float(theta), int(m)
        self.taken = np.zeros(len(self.r), bool)
        self.count = np.zeros(len(self.r), np.int64)        # selected entries of each entry's category
        self.maxcos = np.full(len(self.r), -np.inf)
        self.n = 0

    def eligible(self):
        e = self.ok & ~self.taken
        return e & (self.count < self.m) if self.m > 0 else e

    def values(self):
        v = (1.0 - self.theta) * self.r
        if self.n > 0 and self.theta != 0.0:
            v = v - self.theta * self.maxcos
        return v

    def take(self, j):
        self.taken[j] = True
        self.count += self.cate == self.cate[j]
        self.maxcos = np.maximum(self.maxcos, (self.w @ self.w[j]) * (self.inv * self.inv[j]))
        self.n += 1


def select(ids, s, w, inv, cate, K, theta, m):
    """The pool positions picked, in order (fewer than K when the eligible entries run out): the largest value wins,
    equal values -> lower position."""
    row, picks = _Row(ids, s, w, inv, cate, theta, m), []
    for _ in range(K):
        e = row.eligible()
        if not e.any():
            break
        v = np.where(e, row.values(), -np.inf)
        j = int(np.flatnonzero(e & (v == v[e].max()))[0])
        picks.append(j)
        row.take(j)
    return picks


def replay(ids, s, w, inv, cate, theta, m, picks):
    """Teacher-forced check of a selection `picks` (pool positions): for each step, with the history of the picks before
    it, (max eligible value - value of the pick) in fp64 and whether the pick was eligible -> (regret [n], was_eligible
    [n], more) -- more: whether an eligible entry is left after the last pick (a list may end early only when not)."""
    row = _Row(ids, s, w, inv, cate, theta, m)
    regret, was = np.zeros(len(picks)), np.zeros(len(picks), bool)
    for t, j in enumerate(picks):
        e, v = row.eligible(), row.values()
        was[t] = bool(e[j])
        regret[t] = (v[e].max() if e.any() else -np.inf) - v[j]
        row.take(j)
    return regret, was, bool(row.eligible().any())


def positions(pool_ids, out_ids):
    """Pool positions of one row's returned ids (the -1 padding at the end dropped); the ids must come from the pool,
    each once."""
    pool_ids, out = np.asarray(pool_ids), np.asarray(out_ids)
    n = int((out >= 0).sum())
    assert np.all(out[n:] == -1), out
    picks = []
    for g in out[:n]:
        at = np.flatnonzero(pool_ids == g)
        assert len(at) == 1, (int(g), at)
        picks.append(int(at[0]))
    assert len(set(picks)) == len(picks), picks
    return picks


def capped_ranking(s, cate, K, m, ok=None):
    """Brute force over ALL items of a table: walk them by score (higher first, ties -> lower id) and keep an item while
    fewer than m kept ones share its category -> the first K kept ids."""
    s = np.asarray(s, np.float64)
    ok = np.isfinite(s) if ok is None else ok & np.isfinite(s)
    order = [i for i in np.lexsort((np.arange(len(s)), -np.where(ok, s, 0.0))) if ok[i]]
    kept, per = [], {}
    for i in order:
        c = int(cate[i])
        if m == 0 or per.get(c, 0) < m:
            kept.append(int(i))
            per[c] = per.get(c, 0) + 1
            if len(kept) == K:
                break
    return kept

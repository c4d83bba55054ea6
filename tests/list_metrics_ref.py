"""The fp64 restatement of tlsan_list_metrics (include/tlsan.h), row by row, from the same fp32 vec / inv inputs the
kernel is given, and of ListMetricCounters.result.  Plain numpy loops: clarity over speed, for test-sized inputs.

Tolerance (derived, not measured): an fp32 dot of d terms, one product with fl(inv_i inv_j) and a double accumulation give
|cos - cos64| <= (d + 3) 2^-24 (1 + O(d 2^-24)) per pair, and the same for the mean over the pairs, hence for ILD; where
inv is the kernel's own and the reference norms are formed in fp64 add (d + 4) 2^-24.  Both are under rerank_ref.tau(d) =
8 d 2^-24, the bound the tests use for ILD."""
import numpy as np


def row(ids, w, inv, cate, label=None, weight=None):
    """One list -> dict(n, pair_cos, ild, n_cate, max_cate, hit_pos, weight_sum): ids [K], w [K, d], inv [K], cate [K],
    label an id or None, weight [K] or None."""
    ids = np.asarray(ids)
    v = [j for j in range(len(ids)) if ids[j] >= 0]
    w64, inv64 = np.asarray(w, np.float64), np.asarray(inv, np.float64)
    n = len(v)
    cos = (w64[v] @ w64[v].T) * np.outer(inv64[v], inv64[v]) if n else np.zeros((0, 0))
    pair = float(np.triu(cos, 1).sum())                              # the pairs i < j of the valid entries
    cats = [int(np.asarray(cate)[j]) for j in v]
    hit = -1
    if label is not None and label >= 0:
        for j in v:
            if ids[j] == label:
                hit = j
                break
    ws = 0.0
    if weight is not None:
        for j in v:
            ws += float(np.asarray(weight)[j])
    return dict(n=n, pair_cos=pair, ild=1.0 - pair / (n * (n - 1) / 2.0) if n >= 2 else float("nan"),
                n_cate=len(set(cats)), max_cate=max([cats.count(c) for c in set(cats)] + [0]), hit_pos=hit, weight_sum=ws)


def rows(ids, w, inv, cate, labels=None, weight=None):
    """Lists ids [B, K] (w [B, K, d], inv / cate / weight [B, K], labels [B]) -> dict of [B] arrays."""
    out = [row(ids[b], w[b], inv[b], cate[b], None if labels is None else int(labels[b]),
               None if weight is None else weight[b]) for b in range(len(ids))]
    return {k: np.array([o[k] for o in out], np.float64 if k in ("pair_cos", "ild", "weight_sum") else np.int64)
            for k in out[0]}


def exposure(ids, n_items):
    ids = np.asarray(ids).reshape(-1)
    return np.bincount(ids[(ids >= 0) & (ids < n_items)], minlength=n_items).astype(np.int64)


def gini(x):
    """Gini coefficient of the counts x over all their items, by its definition as the mean absolute difference over
    twice the mean: sum_ij |x_i - x_j| / (2 I sum x)."""
    x = np.asarray(x, np.float64)
    return float(np.abs(x[:, None] - x[None, :]).sum() / (2.0 * len(x) * x.sum()))


def result(m, k, expo=None):
    """ListMetricCounters.result from the rows' measurements m (rows' dict) of lists of length k and the exposure counts."""
    n, hit = m["n"], m["hit_pos"]
    two, one = n >= 2, n >= 1
    mean = lambda x: float(np.sum(x) / len(x)) if len(x) else float("nan")
    found = hit >= 0
    out = {"ILD@%d" % k: mean(m["ild"][two]), "categories@%d" % k: mean(m["n_cate"][one].astype(np.float64)),
           "max_per_category": int(m["max_cate"].max()) if len(n) else 0,
           "HR@%d" % k: float(found.sum()) / len(n),
           "NDCG@%d" % k: float(np.sum(1.0 / np.log2(hit[found] + 2.0))) / len(n),
           "MRR@%d" % k: float(np.sum(1.0 / (hit[found] + 1.0))) / len(n),
           "novelty@%d" % k: float(m["weight_sum"].sum() / n.sum()) if n.sum() else float("nan"),
           "coverage@%d" % k: float("nan"), "gini@%d" % k: float("nan"),
           "rows": len(n), "short_rows": int((n < k).sum())}
    if expo is not None:
        out["coverage@%d" % k] = float((np.asarray(expo) > 0).sum()) / len(expo)
        out["gini@%d" % k] = gini(expo) if np.sum(expo) else float("nan")
    return out


def take(m, sel):
    return {k: v[sel] for k, v in m.items()}

"""Numpy float64 reference of the clustered item index (tlsan_cluster_assign / _means / _probe, ClusteredIndex): the
nearest centroid with its margin, the segment means, the probe order, Lloyd's iterations from given train_ids / init_ids
and recall.  Independent of the library: nothing here is imported from tlsan_amd."""
import numpy as np

U32 = 2.0 ** -24


def bound(d, xn, cn):
    """The standard bound of an fp32 dot product of length d, with the half norm's and the subtraction's roundings:
    2 (d + 2) 2^-24 (|x| |c| + |c|^2 / 2); xn, cn: the norms (broadcast)."""
    return 2.0 * (d + 2) * U32 * (xn * cn + 0.5 * cn * cn)


def values(x, cent):
    """v[n, j] = x_n . c_j - |c_j|^2 / 2 in float64."""
    x, cent = np.asarray(x, np.float64), np.asarray(cent, np.float64)
    return x @ cent.T - 0.5 * (cent * cent).sum(1)[None, :]


def assign(x, cent):
    """-> (assign [N] (argmax of values, ties -> the lower j, a row whose best is NaN -> 0), dist [N] = max(|x|^2 - 2 best,
    0), sure [N] bool: the gap between the row's two best values exceeds the fp32 bound (each of the two values errs by
    at most half of its centroid's bound), so an fp32 assignment must agree; err [N]: the bound at the row's centroid)."""
    x, cent = np.asarray(x, np.float64), np.asarray(cent, np.float64)
    v = values(x, cent)
    N, C = v.shape
    vv = np.where(np.isnan(v), -np.inf, v)
    a = np.argmax(vv, 1)                                   # (numpy: the first of equals)
    best = vv[np.arange(N), a]
    xn, cn = np.sqrt((x * x).sum(1)), np.sqrt((cent * cent).sum(1))
    d = x.shape[1]
    with np.errstate(invalid="ignore"):
        bnd = bound(d, xn[:, None], cn[None, :])
        if C > 1:
            rest = vv.copy()
            rest[np.arange(N), a] = -np.inf
            second = np.argmax(rest, 1)
            gap = best - rest[np.arange(N), second]
            sure = gap > 0.5 * (bnd[np.arange(N), a] + bnd[np.arange(N), second])   # (each value's own error: half the bound)
        else:
            sure = np.ones(N, bool)
        nan_row = np.isnan(x).any(1)
        a = np.where(nan_row, 0, a)
        sure = sure | nan_row
        dist = np.maximum((x * x).sum(1) - 2.0 * best, 0.0)
        err = bnd[np.arange(N), a]
    return a.astype(np.int64), dist, sure, err


def means(x, order, seg_off, cent):
    """cent with row j replaced by float32(mean in float64 of x[order[seg_off[j] : seg_off[j + 1]]]), the sum formed row
    after row in the order given; empty: untouched."""
    out = np.array(cent, np.float32)
    x = np.asarray(x, np.float64)
    for j in range(len(seg_off) - 1):
        rows = np.asarray(order[seg_off[j]:seg_off[j + 1]], np.int64)
        if len(rows):
            acc = np.zeros(x.shape[1])
            for r in rows:
                acc = acc + x[r]
            out[j] = (acc / len(rows)).astype(np.float32)
    return out


def probe_scores(q, cent, scale=None, bias=None):
    s = np.asarray(q, np.float64) @ np.asarray(cent, np.float64).T
    if scale is not None:
        s = s * np.asarray(scale, np.float64)[None, :]
    if bias is not None:
        s = s + np.asarray(bias, np.float64)[None, :]
    return s


def probe_order(s, full=None):
    """The lists of one row in probe order from its scores s [C]: higher first, equal (+0 == -0) -> the lower list, NaN
    last; full [C] bool: the lists that have items (None: all)."""
    ids = np.arange(len(s)) if full is None else np.nonzero(full)[0]
    v = np.asarray(s, np.float64)[ids]
    nan = np.isnan(v)
    return ids[np.lexsort((ids, -(np.where(nan, 0.0, v) + 0.0), nan))]


def probe(q, cent, P, scale=None, bias=None, list_off=None):
    """row_lists [B, P] int64, -1 in the slots left over."""
    s = probe_scores(q, cent, scale, bias)
    full = None if list_off is None else np.diff(np.asarray(list_off, np.int64)) > 0
    out = np.full((s.shape[0], P), -1, np.int64)
    for b in range(s.shape[0]):
        o = probe_order(s[b], full)[:P]
        out[b, :len(o)] = o
    return out


def probe_sure(q, cent, P, scale=None, bias=None, list_off=None):
    """[B, P] bool: slot p of the row is decided beyond fp32 rounding -- the reference's candidate of that slot lies
    further than the bound from every other candidate (so exactly p candidates come out ahead of it in fp32 too), or the
    slot is past the candidates (the fill).  A score errs by at most (d + 2) 2^-24 (|q| |c| |scale| + |bias|): the dot
    product's bound and the two roundings of the score; two candidates straddle a boundary within the bound when the
    intervals of that width around their scores meet."""
    q, cent = np.asarray(q, np.float64), np.asarray(cent, np.float64)
    s = probe_scores(q, cent, scale, bias)
    full = None if list_off is None else np.diff(np.asarray(list_off, np.int64)) > 0
    d = q.shape[1]
    qn, cn = np.sqrt((q * q).sum(1)), np.sqrt((cent * cent).sum(1))
    sc = np.ones(len(cent)) if scale is None else np.abs(np.asarray(scale, np.float64))
    bi = np.zeros(len(cent)) if bias is None else np.abs(np.asarray(bias, np.float64))
    sure = np.ones((len(q), P), bool)
    for b in range(len(q)):
        o = probe_order(s[b], full)
        e = (d + 2) * U32 * (qn[b] * cn[o] * sc[o] + bi[o])
        v = np.where(np.isnan(s[b][o]), -np.inf, s[b][o])
        below = np.concatenate([np.maximum.accumulate((v + e)[::-1])[::-1][1:], [-np.inf]])   # the highest a later one can come out
        above = np.concatenate([[np.inf], np.minimum.accumulate(v - e)[:-1]])                 # the lowest an earlier one can
        ok = (v - e > below) & (v + e < above)
        n = min(P, len(o))
        sure[b, :n] = ok[:n]
    return sure


def fit(x, init_rows, iters):
    """Lloyd on x [n, d] from the centroids x[init_rows]: an iteration is one assignment and one means (rounded to float32,
    as the library holds its centroids); it stops when no assignment changed -> (cent float32, assign of the last
    iteration, objective list, margin: the smallest gap between a row's two best values over all iterations, in units of
    the fp32 bound at the row's centroid -- above 1: every assignment was decided beyond the bound)."""
    x = np.asarray(x, np.float32)
    cent = x[np.asarray(init_rows)].copy()
    objective, prev, margin = [], None, np.inf
    for _ in range(iters):
        a, dist, sure, err = assign(x, cent)
        if len(cent) > 1:
            v = np.sort(values(x, cent), 1)
            margin = min(margin, float(((v[:, -1] - v[:, -2]) / err).min()))
        objective.append(float(dist.sum()))
        if prev is not None and np.array_equal(a, prev):
            break
        prev = a
        order = np.argsort(a, kind="stable")
        seg = np.concatenate([[0], np.cumsum(np.bincount(a, minlength=len(cent)))])
        cent = means(x, order, seg, cent)
    return cent, prev, objective, margin


def recall(approx_ids, exact_ids):
    """Mean over the rows of |approx & exact| / |exact| on the valid (>= 0) ids."""
    vals = []
    for a, e in zip(np.asarray(approx_ids), np.asarray(exact_ids)):
        e = set(int(v) for v in e if v >= 0)
        if e:
            vals.append(len(e & set(int(v) for v in a if v >= 0)) / len(e))
    return float(np.mean(vals)) if vals else float("nan")


def planted(I, d, centres, seed, noise=0.3):
    """I vectors around `centres` planted centres ~ N(0, 1) with N(0, noise^2) noise -> (x float32 [I, d], label [I])."""
    rng = np.random.RandomState(seed)
    mu = rng.randn(centres, d)
    lab = rng.randint(0, centres, I)
    return (mu[lab] + noise * rng.randn(I, d)).astype(np.float32), lab

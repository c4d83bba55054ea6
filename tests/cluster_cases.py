"""The fixtures of the clustered index's kernel tests, shared by tests/test_cluster_cpu.py (which checks the reference
alone against the 1 % cap on excused results) and tests/test_gpu_cluster.py (which runs the kernels on them): seeded
Gaussians at the tile edges.

Probe cases.  A slot of a row is excused when its candidate lies within the fp32 bound of another one
(cluster_ref.probe_sure); at most 1 % of a case's slots may be.  With plain N(0, 1) data the bound grows like
(d + 2) sqrt(d) against the spacing of the scores, so the full cross of C and P runs at d = 64 (0.5 % of the slots at C = 130,
P = 64; the same data at d = 256 would excuse 4 %).  d = 128 and 256 run the sizes with more than one centroid tile under a
wide bias (standard deviation 10 sqrt(d), ten times the products'), where the spacing is the bias's and the bound stays the
product's: the scan, the MFMA chain of that d and the two roundings of the score all still decide the order."""
import numpy as np

DS = (64, 128, 256)
ASSIGN_N = (600, 1, 15, 16, 17)        # (600 first: the others are compared with its rows)
ASSIGN_C = (1, 7, 16, 17, 130)
PROBE_C = (1, 7, 17, 130)
PROBE_P = (1, 8, 9, 64)
PROBE_B = 48


def gauss(n, d, seed):
    return np.random.RandomState(seed).randn(n, d).astype(np.float32)


def assign_case(d, nc):
    """(x [600, d], cent [nc, d])"""
    return gauss(600, d, 0), gauss(nc, d, 100 + nc)


def probe_cases(d):
    """yields (name, q [48, d], cent [C, d], P, kw) -- kw: the scale / bias / list_off of the call"""
    q = gauss(PROBE_B, d, 21)
    for nc in PROBE_C if d == 64 else (17, 130):
        cent = gauss(nc, d, 200 + nc)
        rng = np.random.RandomState(300 + nc)
        scale, bias = rng.uniform(0.5, 2.0, nc).astype(np.float32), rng.randn(nc).astype(np.float32)
        sizes = rng.randint(0, 3, nc)                                   # about a third of the lists are empty
        off = np.concatenate([[0], np.cumsum(sizes)])
        wide = (bias * 10.0 * np.sqrt(d)).astype(np.float32)
        for P in PROBE_P if d == 64 else (8, 64):
            if d == 64:
                forms = (("plain", dict()), ("scale+bias", dict(scale=scale, bias=bias)), ("bias+off", dict(bias=bias, list_off=off)),
                         ("all", dict(scale=scale, bias=bias, list_off=off)))
            else:
                forms = (("wide", dict(bias=wide)), ("wide+all", dict(scale=scale, bias=wide, list_off=off)))
            for name, kw in forms:
                yield "d%d C%d P%d %s" % (d, nc, P, name), q, cent, P, kw


def live_lists(cent, kw):
    return len(cent) if "list_off" not in kw else int((np.diff(kw["list_off"]) > 0).sum())


# The planted table of the fit test: I = 600 items around 12 centres ~ N(0, 1).  The category half of an item's vector is
# its centre's (the category IS the planted label), the item half the centre's plus N(0, 0.3^2) noise.  Lloyd from 12 random
# rows starts with several rows of one planted cluster, so it splits clusters, and an item near such a cut can sit within
# the fp32 bound of it; of the seeds tried (table 0..2, index 1234..1263) this pair keeps every assignment of every
# iteration furthest from the bound: the smallest gap is 0.0146, 20 times the bound (tests/test_cluster_cpu.py checks it).
PLANTED_I, PLANTED_D, PLANTED_LISTS, PLANTED_SEED, FIT_SEED = 600, 64, 12, 2, 1262


def planted_table():
    """(vec [600, 64] float32: the item vectors, item_half [600, 32], cate_rows [12, 32], label [600])"""
    from tests import cluster_ref as cref
    x, lab = cref.planted(PLANTED_I, PLANTED_D, PLANTED_LISTS, PLANTED_SEED)
    mu = np.random.RandomState(PLANTED_SEED).randn(PLANTED_LISTS, PLANTED_D)          # (planted's own first draw: the centres)
    half = PLANTED_D // 2
    cate = mu[:, half:].astype(np.float32)
    return np.concatenate([x[:, :half], cate[lab]], 1), x[:, :half], cate, lab


def fit_draws(count, nlists, seed, train_size=None):
    """The training ids and the initial rows as ClusteredIndex documents them -> (train_ids sorted, init_ids)."""
    rng = np.random.default_rng(seed)
    n = min(count, train_size or 256 * nlists)
    train = np.sort(rng.choice(np.arange(count, dtype=np.int64), n, replace=False))
    return train, train[rng.choice(n, nlists, replace=False)]

"""The cases of tests/test_gpu_index.py: for every form tlsan_batch_index builds a batch's destination index in, the smallest
shapes on both sides of each edge.  A case names the form it was written for (`plan`, every field of tlsan_index_plan):
tests/test_index_ref_cpu.py asserts that on the host, the GPU test again before it builds.  No GPU, no torch.

Thresholds the shapes are written around (csrc/tlsan_api_plan.hip, tlsan_index_args.h, tlsan_state.h): tables of 65 536 rows
are sorted instead of counted (users: batches up to 4096 samples; items: with category segments), 2048 categories take
category segments, more than 32 samples per category list them, scan chunks hold 4096 rows and more than 16 of them take the
two-level scan, use slots come in blocks of 4096, rows with more than 48 uses are hot and up to 64 of them are listed,
batches of more than 16 samples and at most 256 groups are ranked, windows longer than 10 are streamed."""
import numpy as np

from tests.helpers import random_batch

LAZY = 0x100          # TLSAN_INDEX_FOR_LAZY_SGD
AP_HOT, AP_HOT_CAP = 48, 64
PLAN_FIELDS = ("cseg", "uc_list", "usort", "isort", "sparse", "rank", "by_window", "two_level")


class Case:
    def __init__(self, name, make, B, Sn, lazy, plan, U=50, I=40, C=7, Ls=10, d=64):
        self.name, self.make, self.B, self.Sn, self.lazy = name, make, B, Sn, lazy
        self.cfg = dict(U=U, I=I, C=C, Ls=Ls, d=d)
        self.plan = dict(dict.fromkeys(PLAN_FIELDS, 0), **plan)
        assert set(self.plan) == set(PLAN_FIELDS)
        if lazy:
            self.name += "-lazy"

    @property
    def flags(self):
        return LAZY if self.lazy else 0

    def batch(self, cfg):
        """(batch, item -> category map) of the case for the config made from self.cfg"""
        b, cat = self.make(cfg, self.B, self.Sn)
        assert len(b["u"]) == self.B and np.asarray(b["hist_i_new"]).reshape(self.B, -1).shape[1] == self.Sn
        for k, n in (("u", cfg["user_count"]), ("i", cfg["item_count"]), ("hist_i", cfg["item_count"]),
                     ("hist_i_new", cfg["item_count"]), ("u_cate", cfg["cate_count"])):
            assert b[k].size == 0 or (0 <= b[k].min() and b[k].max() < n), k      # every id inside its table
        return b, cat


def rnd(seed):
    return lambda cfg, B, Sn: random_batch(cfg, B=B, Sn=Sn, seed=seed)


def edit(seed, fn):
    """a random batch changed in place by fn(b, cfg, rng)"""
    def make(cfg, B, Sn):
        b, cat = random_batch(cfg, B=B, Sn=Sn, seed=seed)
        fn(b, cfg, np.random.RandomState(seed + 1000))
        return b, cat
    return make


def _repad(b):
    """ids past the lengths back to the padding zero (after an edit of whole id arrays)"""
    Ls, Sn = b["hist_i"].shape[1], b["hist_i_new"].shape[1]
    b["hist_i"][np.arange(Ls)[None, :] >= b["sl"][:, None]] = 0
    b["hist_i_new"][np.arange(Sn)[None, :] >= b["sl_new"][:, None]] = 0


CASES = []
add = CASES.append
both = (False, True)

# ---- counted, dense and lazy (lazy: the user offsets are written for the used rows only)
for lazy in both:
    sp = 4 if lazy else 0
    add(Case("counted", rnd(1), 37, 3, lazy, dict(sparse=sp, rank=1)))
    add(Case("counted-B1", rnd(2), 1, 0, lazy, dict(sparse=sp)))
    add(Case("counted-U1", rnd(3), 37, 3, lazy, dict(sparse=sp, rank=1), U=1))


# ---- chunk edges of the scan: the thread of row n - 1 writes n_uniq and off[n]
def _last_row(used):
    def fn(b, cfg, rng):
        U, I = cfg["user_count"], cfg["item_count"]
        for k in ("hist_i", "hist_i_new", "i"):
            b[k][b[k] == I - 1] = I - 2
        b["u"][b["u"] == U - 1] = U - 2
        if used:
            b["i"][5] = I - 1
            b["u"][7] = U - 1
    return fn


for lazy in both:
    sp = 4 if lazy else 0
    for n in (4095, 4096, 4097, 8193):
        for used in (True, False):
            add(Case("chunk-%d-%s" % (n, "last" if used else "nolast"), edit(10 + n % 7, _last_row(used)), 37, 3, lazy,
                     dict(sparse=sp, rank=1), U=n, I=n))


def _row0_only(b, cfg, rng):
    for k in ("hist_i", "hist_i_new", "i", "u", "u_cate"):
        b[k][:] = 0


for lazy in both:
    add(Case("chunk-row0-only", edit(20, _row0_only), 37, 3, lazy, dict(sparse=4 if lazy else 0, rank=1), U=4097, I=4097))

# ---- the two-level scan: 16 chunks take one launch, one row more takes two
for lazy in both:
    sp = 4 if lazy else 0
    add(Case("scan-16-chunks", rnd(30), 37, 3, lazy, dict(sparse=sp, rank=1, two_level=0), I=16 * 4096))
    add(Case("scan-16-chunks+1", rnd(31), 37, 3, lazy, dict(sparse=sp, rank=1, two_level=1), I=16 * 4096 + 1))


# ---- flag_user: 256-row pieces of a large user table that is counted (4097 samples: the sort is refused)
def _users_in(*ranges):
    def fn(b, cfg, rng):
        pool = np.concatenate([np.arange(lo, hi) for lo, hi in ranges])
        b["u"][:] = rng.choice(pool, len(b["u"]))
    return fn


_U = 70001
_LASTP = (_U - 1) // 256 * 256
_flag_plan = dict(uc_list=1, two_level=1)      # (257 groups: no ranking with windows in registers)
add(Case("flags-first-last-piece", edit(40, _users_in((0, 256), (_LASTP, _U))), 4097, 1, True, dict(_flag_plan, sparse=4), U=_U))
add(Case("flags-adjacent-pieces", edit(41, _users_in((512, 1024))), 4097, 1, True, dict(_flag_plan, sparse=4), U=_U))
add(Case("flags-one-piece", edit(42, _users_in((1000, 1011))), 4097, 1, True, dict(_flag_plan, sparse=4), U=_U))
add(Case("flags-65536", edit(43, _users_in((255, 257), (65535, 65536))), 4097, 1, True, dict(_flag_plan, sparse=4, two_level=0), U=65536))   # (16 chunks)
add(Case("flags-first-last-piece", edit(40, _users_in((0, 256), (_LASTP, _U))), 4097, 1, False, dict(_flag_plan), U=_U))


# ---- the user side from the bucket sort (usort_block)
def _distinct(b, cfg, rng):
    b["u"][:] = rng.permutation(cfg["user_count"])[:len(b["u"])]


def _repeat3000(b, cfg, rng):
    b["u"][rng.permutation(len(b["u"]))[:3000]] = 33333


def _ends(b, cfg, rng):
    b["u"][::3] = 0
    b["u"][1::3] = cfg["user_count"] - 1


def _one_bucket(b, cfg, rng):        # (buckets hold 64 ids at 65 536 users, 128 at 70 001)
    b["u"][:] = 640 + rng.randint(0, 64, len(b["u"]))


for U in (65536, 70001):
    for B in (1, 2, 1023, 1024, 1025, 4096):
        add(Case("usort-%d-B%d" % (U, B), rnd(50 + B % 11), B, 1, True,
                 dict(usort=1, sparse=4, uc_list=int(B > 32 * 7), rank=int(B > 16)), U=U))
    for tag, fn in (("distinct", _distinct), ("repeat3000", _repeat3000), ("ends", _ends), ("one-bucket", _one_bucket)):
        add(Case("usort-%d-%s" % (U, tag), edit(60, fn), 4096, 1, True, dict(usort=1, sparse=4, uc_list=1, rank=1), U=U))
add(Case("usort-ends-B2", edit(61, _ends), 2, 1, True, dict(usort=1, sparse=4), U=70001))


# ---- the item side from the partitioned counting sort (k_isort_*): 2048 categories, 16 use slots per sample
def _skip_bucket(b, cfg, rng):       # (200 000 items: 49 buckets of 4096 ids) nothing in bucket 3
    for k in ("hist_i", "hist_i_new", "i"):
        b[k][(b[k] >> 12) == 3] += 4096
    _repad(b)


def _last_bucket(b, cfg, rng):
    I = cfg["item_count"]
    lo = (I - 1) >> (10 if I == 65536 else 12) << (10 if I == 65536 else 12)
    for k in ("hist_i", "hist_i_new", "i"):
        b[k][...] = lo + b[k] % (I - lo)
    b["i"][0] = I - 1
    _repad(b)


_isort = dict(cseg=1, isort=1, sparse=5, rank=1)
for I in (65536, 200000):
    for B, blocks in ((256, 1), (512, 2), (2048, 8), (2049, 9)):
        assert -(-B * 16 // 4096) == blocks
        add(Case("isort-%d-%dblk" % (I, blocks), rnd(70 + blocks), B, 5, True, _isort, I=I, C=2048))
    add(Case("isort-%d-last-bucket" % I, edit(80, _last_bucket), 256, 5, True, _isort, I=I, C=2048))
add(Case("isort-empty-bucket", edit(81, _skip_bucket), 512, 5, True, _isort, I=200000, C=2048))
add(Case("isort-usort", rnd(82), 512, 5, True, dict(_isort, usort=1), U=70001, I=200000, C=2048))

# ---- category segments with counted items, and one category fewer: none
for lazy in both:
    add(Case("cseg-counted", rnd(90), 37, 3, lazy, dict(cseg=1, sparse=5 if lazy else 0, rank=1), I=5000, C=2048))
    add(Case("cseg-off-2047", rnd(91), 37, 3, lazy, dict(cseg=0, sparse=4 if lazy else 0, rank=1), I=5000, C=2047))


# ---- hot rows: more than AP_HOT uses; listed while there are at most AP_HOT_CAP
def _hot(counts):
    """candidates: id k gets counts[k] uses; everything else is cold (ids from 100 on, a few uses each); one window
    entry per sample, no session entries"""
    def fn(b, cfg, rng):
        B, I = len(b["u"]), cfg["item_count"]
        cold = 100 + np.arange(2 * B) % (I - 100)
        b["sl"][:] = 1
        b["sl_new"][:] = 0
        b["hist_i"][:, 0] = cold[:B]
        b["i"][:] = cold[B:]
        pos = 0
        for k, n in enumerate(counts):
            b["i"][pos:pos + n] = k
            pos += n
        assert pos <= B and len(counts) < 100
        _repad(b)
    return fn


for tag, lazy, kw, plan in (("counted", False, dict(I=400), dict()),
                            ("sorted", True, dict(I=65536, C=2048), dict(cseg=1, isort=1, sparse=5))):
    add(Case("hot-%s-48-49" % tag, edit(100, _hot([AP_HOT, AP_HOT + 1])), 128, 1, lazy, dict(plan, rank=1), **kw))
    for nhot in (AP_HOT_CAP, AP_HOT_CAP + 1):
        add(Case("hot-%s-%d-rows" % (tag, nhot), edit(101, _hot([AP_HOT + 1] * nhot)), 3250, 1, lazy,
                 dict(plan, rank=1, uc_list=0 if kw.get("C") else 1), **kw))


# ---- the samples of every category (k_uc_fill): listed from 33 samples per category on
def _cates(pick):
    def fn(b, cfg, rng):
        b["u_cate"][:] = pick(rng, len(b["u"]))
    return fn


add(Case("uclist-96-not-listed", rnd(110), 96, 3, False, dict(uc_list=0, rank=1), C=3))
add(Case("uclist-97-listed", rnd(111), 97, 3, False, dict(uc_list=1, rank=1), C=3))
add(Case("uclist-empty-category", edit(112, _cates(lambda rng, B: 2 * rng.randint(0, 2, B))), 97, 3, False, dict(uc_list=1, rank=1), C=3))
add(Case("uclist-one-category", edit(113, _cates(lambda rng, B: np.ones(B, np.int64))), 97, 3, False, dict(uc_list=1, rank=1), C=3))
for lazy in both:
    add(Case("uclist-600-shared", rnd(114), 600, 3, lazy, dict(uc_list=1, rank=1, sparse=4 if lazy else 0), C=3))


# ---- the ranking of the batch: keyed by window where windows are streamed, by session and window where they sit in registers
def _sessions(pick):
    def fn(b, cfg, rng):
        b["sl_new"][:] = pick(rng, len(b["u"]))
        b["hist_i_new"][...] = rng.randint(0, cfg["item_count"], b["hist_i_new"].shape)
        _repad(b)
    return fn


for Ls, by_window in ((33, 1), (10, 0)):
    for B in (16, 17, 32, 33, 250):
        add(Case("rank-Ls%d-B%d" % (Ls, B), rnd(120 + B % 13), B, 4, False,
                 dict(rank=int(B > 16), by_window=by_window if B > 16 else 0, uc_list=int(B > 32 * 7)), Ls=Ls))
_reg = dict(rank=1, by_window=0, uc_list=1)
add(Case("rank-reg-no-heavy", edit(130, _sessions(lambda rng, B: rng.randint(0, 2, B))), 250, 4, False, _reg))           # H = 0
add(Case("rank-reg-all-heavy", edit(131, _sessions(lambda rng, B: rng.randint(2, 5, B))), 250, 4, False, _reg))         # H = 16
add(Case("rank-reg-all-heavy-B32", edit(132, _sessions(lambda rng, B: rng.randint(2, 5, B))), 32, 4, False, dict(_reg, uc_list=0)))
add(Case("rank-reg-mix", edit(133, _sessions(lambda rng, B: np.where(np.arange(B) % 7 == 3, 3, rng.randint(0, 2, B)))), 250, 4,
         False, _reg))                                                                                                    # 36 heavy samples, 16 groups
# (small d = 128 batches run as 8-sample groups in the batch's own order: no ranking is written)
add(Case("rank-d128-small-groups", rnd(134), 33, 4, False, dict(rank=0), d=128))

assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}

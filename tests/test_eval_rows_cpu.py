"""The driver's evaluation passes (tlsan_amd/train.py: EvalRows and the five evaluations written against it) without a
GPU: a stub model whose per-row results are fixed functions of a row's own contents, over one process (whole launches
and shares at world 1) and over 2 and 3 gloo processes.  What is compared are exact integers -- pairs ranked right, the
P@k / R@k hit counters, the two rank histograms -- and the recommendation arrays, each against the value computed
straight from the test set's arrays."""
import inspect
import types

import numpy as np
import pytest
import torch

from tests.ranks import run_ranks
from tlsan_amd import train as T
from tlsan_amd.input import PackedSet
from tlsan_amd.model import KS, TopKCounters

N, BS, ITEMS, NEG, SEED, TOPK = 233, 7, 64, 20, 5, 4    # 33 test batches of 7 rows and one of 2: at world 3 a rank has none
CFG = dict(test_batch_size=BS, Ls=3, item_count=ITEMS)


def _test_set():
    rng = np.random.RandomState(1)
    hist_off = np.arange(N + 1) * 2
    return PackedSet(1000 + np.arange(N), hist_off, rng.randint(0, ITEMS, 2 * N), np.ones(2 * N), np.arange(N + 1),
                     rng.randint(0, ITEMS, N), np.zeros(N), pos=rng.randint(0, ITEMS, N), neg=rng.randint(0, ITEMS, N))


def _right(u, i):
    return (u + i) % 3 != 0


def _rank(u, i):
    return (u * 7 + i * 3) % 60


class _Writer:
    def __init__(self):
        self.rows = []

    def add_summary(self, summary=None, global_step=None):
        self.rows.append(summary)


class StubModel:
    """The per-row methods the evaluations call, as fixed functions of a row's (u, i) on CPU tensors; sampled_ranks
    also of the row's index in the test set (row0 + b), so a wrong row0 changes the result."""

    def __init__(self):
        self._topk, self.eval_writer = TopKCounters(), _Writer()
        self.global_step = types.SimpleNamespace(eval=lambda: 0)

    def check_static_overflow(self):
        pass

    def device_batch(self, batch, is_test=True):
        if isinstance(batch, types.SimpleNamespace):
            return batch
        return types.SimpleNamespace(u=torch.as_tensor(np.asarray(batch[0])), i=torch.as_tensor(np.asarray(batch[1])))

    def pairs_ranked_right(self, batch):
        db = self.device_batch(batch)
        return _right(db.u, db.i)

    def label_ranks(self, batch, exclude=None):
        db = self.device_batch(batch)
        return _rank(db.u, db.i).to(torch.int32)

    def sampled_ranks(self, batch, n, seed=0, row0=0, exclude=None):
        db = self.device_batch(batch)
        return ((db.i + row0 + torch.arange(len(db.i)) + seed) % (n + 1)).to(torch.int32)

    def recommend(self, batch, k, exclude=None):
        db = self.device_batch(batch)
        ar = torch.arange(k)[None, :]
        return ((db.u[:, None] * k + ar) % ITEMS).to(torch.int32), (db.u[:, None] + 0.5 * ar).float()


def _expected():
    ts = _test_set()
    u, i, g = ts.u, ts.pos, np.arange(N)
    ranks = _rank(u, i)
    ar = np.arange(TOPK)[None, :]
    return dict(right=int(_right(u, i).sum()), hits=np.array([(ranks < k).sum() for k in KS]),
                sampled=np.bincount((i + g + SEED) % (NEG + 1), minlength=NEG + 1),
                full=np.bincount(ranks, minlength=ITEMS), user=u,
                ids=(u[:, None] * TOPK + ar) % ITEMS, scores=(u[:, None] + 0.5 * ar).astype(np.float32))


class _Recorder:
    """Wraps a metrics function of train.py and keeps the histograms it is given."""

    def __init__(self, fn):
        self.fn, self.hists = fn, []

    def __call__(self, hist, *a):
        self.hists.append(np.asarray(hist).copy())
        return self.fn(hist, *a)


def _evaluate(rows):
    """The five evaluations over `rows` with a fresh stub -> what they computed, as host values."""
    m, ts = StubModel(), rows.test_set
    sampled, full = _Recorder(T.metrics_from_histogram), _Recorder(T.full_ranking_metrics)
    keep = T.metrics_from_histogram, T.full_ranking_metrics
    T.metrics_from_histogram, T.full_ranking_metrics = sampled, full
    try:
        out = dict(auc=T.eval_auc(m, ts, CFG, rows))
        for _ in range(2):                               # (the counters are cumulative: two rounds)
            prec, recall = T.eval_prec_recall(m, ts, CFG, rows)
        T.eval_sampled(m, rows, NEG, SEED, None)
        T.eval_full_ranking(m, rows, None)
        rec = T.recommend_test_set(m, rows, TOPK, None)
    finally:
        T.metrics_from_histogram, T.full_ranking_metrics = keep
    c = m._topk
    out.update(prec=prec, recall=recall, hits_p=c.hits_p.copy(), hits_r=c.hits_r.copy(), n_p=c.n_p, n_r=c.n_r,
               sampled=sampled.hists[-1], full=full.hists[-1], rec=rec,
               tags=[r[0] if isinstance(r, tuple) else [t for t, _ in r] for r in m.eval_writer.rows])
    return out


def _check(got, exp):
    # a unit's float32 mean is within 2^-24 (relative) of its count / length, so the weighted sum is within N * 2^-24 of
    # the count (1e-9: the roundings of the float64 sums, some 1e-14 each)
    assert abs(got["auc"] * N - exp["right"]) <= N * 2.0 ** -24 + 1e-9 and round(got["auc"] * N) == exp["right"]
    assert np.array_equal(got["hits_p"], 2 * exp["hits"]) and np.array_equal(got["hits_r"], 2 * exp["hits"])
    assert got["n_p"] == got["n_r"] == 2 * N                   # (a counted padding row would show here)
    assert got["prec"] == [float(h) / (k * N) for h, k in zip(exp["hits"], KS)]
    assert got["recall"] == [float(h) / N for h in exp["hits"]]
    assert np.array_equal(got["sampled"], exp["sampled"]) and got["sampled"].sum() == N
    assert np.array_equal(got["full"], exp["full"]) and got["full"].sum() == N
    user, ids, scores = got["rec"]
    assert np.array_equal(user, exp["user"]) and np.array_equal(ids, exp["ids"]) and np.array_equal(scores, exp["scores"])
    assert got["tags"][0] == "AUC" and got["tags"][1] == ["P@%d" % k for k in KS] + ["R@%d" % k for k in KS]
    assert got["tags"][3][0] == "HR@1" and got["tags"][4][0] == "Full/HR@1"


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("pad", [False, True])
def test_shares_tile_the_test_set(world, pad):
    ts = _test_set()
    per_rank = [list(T.EvalRows(ts, CFG, rank, world).launches(pad)) for rank in range(world)]
    assert all(len(x) == -(-N // BS) for x in per_rank)      # every rank launches for every batch, rows or not
    covered = np.zeros(N, np.int64)
    for launches in per_rank:
        for rows, real, row0 in launches:
            covered[row0:row0 + real] += 1
            assert 0 <= real <= len(rows[0]) and len(rows[0]) >= 1
            assert np.array_equal(rows[0][:real], ts.u[row0:row0 + real])        # the rows that count are those rows
            assert np.array_equal(rows[1][:real], ts.pos[row0:row0 + real])
    assert (covered == 1).all()
    for b, same_batch in enumerate(zip(*per_rank)):
        n = min(BS, N - b * BS)
        assert sum(real for _, real, _ in same_batch) == n
        if pad:
            assert {len(rows[0]) for rows, _, _ in same_batch} == {-(-n // world)}
    if world == 3:
        assert per_rank[0][-1][1] == 0                         # the last batch's 2 rows leave rank 0 a placeholder


@pytest.mark.parametrize("chunk", [4096, 100, 10])
def test_whole_launches_tile_the_test_set(chunk, monkeypatch):
    monkeypatch.setattr(T, "EVAL_CHUNK", chunk)              # (read when the launches are formed)
    ts = _test_set()
    rows = T.EvalRows(ts, CFG)
    launches = list(rows.launches(True))
    size = max(chunk, BS) // BS * BS
    assert [(real, row0) for _, real, row0 in launches] == [(min(size, N - lo), lo) for lo in range(0, N, size)]
    assert all(len(b[0]) == real for b, real, _ in launches)
    assert sum((rows.units(real) for _, real, _ in launches), []) == [BS] * (N // BS) + [N % BS]
    assert rows.total == N


def test_evaluations_one_process(monkeypatch):
    exp = _expected()
    got = {}
    for chunk in (4096, 100):
        monkeypatch.setattr(T, "EVAL_CHUNK", chunk)
        got[chunk] = _evaluate(T.EvalRows(_test_set(), CFG))
        _check(got[chunk], exp)
    assert got[4096]["auc"] == got[100]["auc"]               # same units (the reference's batches), same float
    share = _evaluate(T.EvalRows(_test_set(), CFG, 0, 1))
    _check(share, exp)
    assert share["auc"] == got[4096]["auc"]                  # at world 1 a share is a reference batch
    quiet = StubModel()
    T.eval_prec_recall(quiet, _test_set(), CFG, summary=False)
    assert quiet.eval_writer.rows == [] and quiet._topk.n_p == N


def _worker(rank, world):
    got = _evaluate(T.EvalRows(_test_set(), CFG, rank, world))
    assert (got["rec"] is None) == (rank != 0)             # rank 0 alone holds (and writes) the recommendations
    if rank == 0:
        _check(got, _expected())


@pytest.mark.parametrize("world", [2, 3])
def test_evaluations_over_gloo(world):
    run_ranks(_worker, world)


def test_drivers_hand_run_the_rows():
    params = list(inspect.signature(T._run).parameters)
    assert "rows" in params and "seen" in params
    assert not [p for p in params if p.startswith("eval") or p.startswith("recommend")]
    for driver in (T.train, T.train_sharded):
        assert "EvalRows" in driver.__code__.co_names or "EvalRows" in driver.__code__.co_freevars
        nested = {c.co_name for c in driver.__code__.co_consts if inspect.iscode(c)}
        assert not [n for n in nested if n.startswith("eval") or n.startswith("recommend") or n == "reduce_sum"], nested

"""GPU tests of candidate scoring and the sampled evaluation (tlsan_score_candidates / tlsan_candidate_ranks /
tlsan_sample_negatives, Model and ShardedModel .score_candidates / .sample_negatives / .sampled_ranks, the driver's
--eval_negatives): against the fp64 oracle, bit for bit against the label's score and the top-K lists, the identity with
the all-items rank, the order's corner cases, the sampler against its definition, sharded against single-GPU."""
import os

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.candidates_ref import reference_negatives
from tests.helpers import (batch_tuple, bits, history_sets, host, label_scores, lazy_model, make_config, model, p32,
                           random_batch, random_params)
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (64, 4), (128, 16), (128, 4)])
def test_candidate_scores_match_oracle(d, H):
    cfg = make_config(U=60, I=700, C=13, d=d, H=H)
    p = p32(random_params(cfg, seed=11))
    b, cat = random_batch(cfg, B=77, Sn=3, seed=12, test=True)
    m = model(cfg, cat, p)
    ref = orc.forward(p, cat, b, H)
    scores = orc.all_item_scores(p, cat, ref["u_t"])
    rng = np.random.RandomState(13)
    cand = rng.randint(0, 700, (77, 37))
    cand[:, 0] = b["i"]
    cand[rng.rand(77, 37) < 0.1] = -1                                  # padding
    got = host(m.score_candidates(batch_tuple(b, True), cand))
    assert got.shape == (77, 37) and got.dtype == np.float32
    pad = cand < 0
    assert pad.sum() > 100 and np.all(got[pad] == -np.inf)
    want = np.take_along_axis(scores, np.maximum(cand, 0), 1)
    assert np.abs(got[~pad] - want[~pad]).max() < 1e-4


@pytest.mark.parametrize("form,table_dtype", [("dense", "f32"), ("dense", "bf16"), ("gather", "f32"), ("gather", "bf16")])
def test_candidate_scores_bitwise_equal_label_and_recommend(form, table_dtype):
    """Lazy L2 (P != 1 after two steps): the label's candidate score equals tlsan_eval_label_scores', and a top-K item's
    equals recommend's, bit for bit -- on a small table and one too large for the rank path's dense item matrix."""
    I = 2000 if form == "dense" else 270000          # gather: I * d * 4 B > 256 MB
    cfg, m = lazy_model(I, table_dtype, 21)
    b, _ = random_batch(cfg, B=200, Sn=3, seed=23, test=True)
    _, _, ut, db = m.forward(batch_tuple(b, True), is_test=True, want_u_t=True)
    slab = label_scores(m, db, ut)
    ids, sc = (host(t) for t in m.recommend(batch_tuple(b, True), 30))
    rng = np.random.RandomState(24)
    cand = np.concatenate([b["i"][:, None], ids, rng.randint(0, I, (200, 9))], 1)
    cand[:, 5::7] = cand[:, 5::7][:, ::-1]          # (columns in another order: the column must not matter)
    got = host(m.score_candidates(batch_tuple(b, True), cand))
    assert np.array_equal(bits(got[:, 0]), bits(slab))
    for r in range(200):
        pos = {g: j for j, g in enumerate(ids[r].tolist())}
        for c in range(1, cand.shape[1]):
            if int(cand[r, c]) in pos:
                assert bits(got[r, c]) == bits(sc[r, pos[int(cand[r, c])]]), (r, c)
    # the same item in every row position and column scores the same
    again = host(m.score_candidates(batch_tuple(b, True), cand[:, ::-1].copy()))
    assert np.array_equal(bits(again[:, ::-1]), bits(got))


@pytest.mark.parametrize("form", ["gather", "dense"])
def test_full_candidate_list_gives_label_rank(form):
    """Every item but the label as candidates: the candidate rank is label_ranks' rank (the gather form exactly; the
    dense rank kernel fuses (acc * P) + bias into one FMA, so rows with an item within an ulp or two of the label may
    differ, as test_topk_consistent_with_label_ranks documents)."""
    from tlsan_amd.model import candidate_ranks
    I = 2000 if form == "dense" else 270000
    cfg, m = lazy_model(I, "f32", 31)
    B = 64 if form == "dense" else 16
    b, _ = random_batch(cfg, B=B, Sn=3, seed=33, test=True)
    ranks = host(m.label_ranks(batch_tuple(b, True)))
    allc = np.arange(I)
    cand = np.stack([np.concatenate([[l], allc[allc != l]]) for l in b["i"]])
    sc = m.score_candidates(batch_tuple(b, True), cand)
    import torch
    ct = torch.as_tensor(cand.astype(np.int32)).to(m.device)
    got = host(candidate_ranks(m.lib, ct, sc, m._stream()))
    if form == "gather":
        assert np.array_equal(got, ranks)
    else:
        bad = got != ranks
        assert bad.sum() <= 2, bad.sum()
        assert np.abs(got - ranks).max() <= 2


def test_candidate_order_corner_cases():
    from tlsan_amd.model import candidate_ranks
    import torch
    cfg = make_config(U=20, I=300, C=5, d=64)
    p = p32(random_params(cfg, seed=41))
    b, cat = random_batch(cfg, B=16, Sn=2, seed=42, test=True)
    for k in ("i", "j", "hist_i", "hist_i_new"):   # item 7 (NaN below) stays out of the inputs: u_t must stay finite
        b[k] = np.where(b[k] == 7, 8, b[k])
    tied = np.array([250, 40, 130, 90, 210])          # bit-identical rows (exact ties)
    p["item_emb"][tied] = p["item_emb"][tied[0]]
    p["item_b"][tied] = p["item_b"][tied[0]]
    cat[tied] = cat[tied[0]]
    p["item_emb"][7] = np.nan
    m = model(cfg, cat, p)

    def rank(cand):
        sc = m.score_candidates(batch_tuple(b, True), cand)
        ct = torch.as_tensor(np.asarray(cand, np.int32)).to(m.device)
        return host(candidate_ranks(m.lib, ct, sc, m._stream())), host(sc)

    # exact ties resolve to the lower id: the label's rank is the number of tied ids below it
    for lab in tied:
        cand = np.tile(np.concatenate([[lab], tied[tied != lab]]), (16, 1))
        r, sc = rank(cand)
        assert np.all(sc == sc[:, :1])
        assert np.all(r == (tied < lab).sum()), (lab, r)
    # a NaN candidate is never ahead; a NaN label is behind every other candidate
    base = np.array([[int(b["i"][r]), 3, 17, 55, 199] for r in range(16)])
    r0, _ = rank(base)
    r1, sc1 = rank(np.concatenate([base, np.full((16, 1), 7)], 1))
    assert np.all(np.isnan(sc1[:, -1])) and np.array_equal(r0, r1)
    r2, _ = rank(np.concatenate([np.full((16, 1), 7), base], 1))
    assert np.all(r2 == 5)
    # repeats of the label's id and padding are not counted
    rep = np.concatenate([base[:, :1], base[:, :1], base[:, 1:3], base[:, :1], np.full((16, 2), -1), base[:, 3:]], 1)
    r3, sc3 = rank(rep)
    assert np.array_equal(r3, r0) and np.all(sc3[:, 5:7] == -np.inf)


def _sampler_case(B, I=22048, seed=51):
    cfg = make_config(U=500, I=I, C=40, d=128)
    b, cat = random_batch(cfg, B=B, Sn=4, seed=seed, test=True)
    return cfg, b, cat


def test_sampler_matches_definition():
    cfg, b, cat = _sampler_case(4096)
    m = model(cfg, cat, p32(random_params(cfg, seed=52)))
    hist = history_sets(b)
    for n, exclude, row0, seed in ((100, "history", 0, 1234), (1000, None, 77, 5), (1, "history", 1 << 40, 2 ** 64 - 1)):
        neg = host(m.sample_negatives(batch_tuple(b, True), n, seed=seed, row0=row0, exclude=exclude))
        assert neg.shape == (4096, n) and neg.dtype == np.int32
        assert (neg >= 0).all() and (neg < 22048).all()
        assert (neg != b["i"][:, None]).all()
        for r in range(0, 4096, 97 if n < 1000 else 401):
            ex = hist[r] if exclude else set()
            assert np.array_equal(neg[r], reference_negatives(22048, b["i"][r], ex, n, seed, row0 + r)), (n, r)
            assert len(set(neg[r].tolist())) == n and not (set(neg[r].tolist()) & ex)
    # per-row lists, ids out of range among them
    lists = [np.array([r, r + 1, -4, 10 ** 6, r]) for r in range(4096)]
    neg = host(m.sample_negatives(batch_tuple(b, True), 50, row0=9, exclude=lists))
    for r in range(0, 4096, 211):
        assert np.array_equal(neg[r], reference_negatives(22048, b["i"][r], {r, r + 1}, 50, 1234, 9 + r))


def test_sampler_independent_of_batch_and_pads():
    cfg, b, cat = _sampler_case(4096)
    m = model(cfg, cat, p32(random_params(cfg, seed=53)))
    full = host(m.sample_negatives(batch_tuple(b, True), 100, row0=1000))
    sub = {k: v[100:137] for k, v in b.items()}
    assert np.array_equal(host(m.sample_negatives(batch_tuple(sub, True), 100, row0=1100)), full[100:137])
    one = {k: v[500:501] for k, v in b.items()}
    assert np.array_equal(host(m.sample_negatives(batch_tuple(one, True), 100, row0=1500)), full[500:501])
    # a 40-item table, N = 50: every eligible item once, then -1
    cfg, b, cat = _sampler_case(37, I=40, seed=54)
    m = model(cfg, cat, p32(random_params(cfg, seed=55)))
    neg = host(m.sample_negatives(batch_tuple(b, True), 50, row0=3))
    for r, h in enumerate(history_sets(b)):
        elig = set(range(40)) - h - {int(b["i"][r])}
        k = len(elig)
        assert set(neg[r, :k].tolist()) == elig and np.all(neg[r, k:] == -1), r
        assert np.array_equal(neg[r], reference_negatives(40, b["i"][r], h, 50, 1234, 3 + r))
    # sampled ranks on such rows: the padding is not counted
    ranks = host(m.sampled_ranks(batch_tuple(b, True), 50, row0=3))
    assert (ranks >= 0).all() and (ranks <= 39).all()


def test_sampled_ranks_compose_the_parts():
    from tlsan_amd.model import sampled_metrics
    cfg, b, cat = _sampler_case(300, I=5000, seed=56)
    p = p32(random_params(cfg, seed=57))
    m = model(cfg, cat, p)
    neg = host(m.sample_negatives(batch_tuple(b, True), 100, row0=20))
    cand = np.concatenate([b["i"][:, None], neg], 1)
    sc = host(m.score_candidates(batch_tuple(b, True), cand)).astype(np.float64)
    want = ((sc[:, 1:] > sc[:, :1]) | ((sc[:, 1:] == sc[:, :1]) & (neg < b["i"][:, None]))).sum(1)
    got = host(m.sampled_ranks(batch_tuple(b, True), 100, row0=20))
    assert np.array_equal(got, want)
    ref = orc.forward(p, cat, b, 8)
    osc = np.take_along_axis(orc.all_item_scores(p, cat, ref["u_t"]), cand, 1)
    assert np.abs(sampled_metrics(got, 100)["MRR"] - sampled_metrics((osc[:, 1:] > osc[:, :1]).sum(1), 100)["MRR"]) < 0.02


def _case():
    cfg = make_config(U=61, I=1501, C=9, d=128)
    p = p32(random_params(cfg, seed=61))
    b, cat = random_batch(cfg, B=48, Sn=3, seed=62, test=True)
    cand = np.random.RandomState(63).randint(-1, 1510, (48, 41))   # padding and ids past the table among them
    cand[:, 0] = b["i"]
    cand[:, 7] = 0
    return cfg, p, b, cat, cand


def _shard_worker(rank, world, out_dir):
    from tlsan_amd.dist import ShardedModel
    from tlsan_amd import train as T
    cfg, p, b, cat, cand = _case()
    m = ShardedModel(cfg, cat, device="cuda:0")
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    n = len(b["u"]) // world
    part = {k: v[rank * n:(rank + 1) * n] for k, v in b.items()}
    res = dict(scores=host(m.score_candidates(batch_tuple(part, True), cand[rank * n:(rank + 1) * n])),
               neg=host(m.sample_negatives(batch_tuple(part, True), 64, seed=9, row0=rank * n)),
               ranks=host(m.sampled_ranks(batch_tuple(part, True), 64, seed=9, row0=rank * n)),
               ranks_none=host(m.sampled_ranks(batch_tuple(part, True), 200, row0=rank * n, exclude=None)))
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    # the drivers: no training, the sampled metrics of the same model over the clothing test set
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    argv = ["--dataset", ds, "--max_epochs", "0", "--quiet", "--eval_negatives", "100", "--eval_topk", "0",
            "--model_dir", os.path.join(out_dir, "r%d" % rank), "--device_input", "0"]
    res = T.train_sharded(T.parse(argv + ["--sharded", "1"]))
    if rank == 0:
        one = T.train(T.parse(argv))
        assert set(res["sampled"]) == set(one["sampled"])
        for k in one["sampled"]:
            assert abs(res["sampled"][k] - one["sampled"][k]) < 1e-12, (k, res["sampled"], one["sampled"])


def test_sharded_candidates_match_model(tmp_path):
    """Against Model on the same launches (each rank's rows as one batch): the forward's u_t can differ in its last bits
    with the launch's batch size, the scoring given u_t cannot."""
    world = 2
    run_ranks(_shard_worker, world, str(tmp_path))
    cfg, p, b, cat, cand = _case()
    m = model(cfg, cat, p)
    got = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    cat_ = lambda k: np.concatenate([g[k] for g in got])
    n = len(b["u"]) // world
    parts = [{k: v[r * n:(r + 1) * n] for k, v in b.items()} for r in range(world)]
    sc = np.concatenate([host(m.score_candidates(batch_tuple(parts[r], True), cand[r * n:(r + 1) * n])) for r in range(world)])
    assert np.array_equal(bits(cat_("scores")), bits(sc))
    assert np.all(sc[(cand < 0) | (cand >= 1501)] == -np.inf)
    assert np.array_equal(cat_("neg"), host(m.sample_negatives(batch_tuple(b, True), 64, seed=9)))
    ranks = [host(m.sampled_ranks(batch_tuple(parts[r], True), 64, seed=9, row0=r * n)) for r in range(world)]
    assert np.array_equal(cat_("ranks"), np.concatenate(ranks))
    ranks = [host(m.sampled_ranks(batch_tuple(parts[r], True), 200, row0=r * n, exclude=None)) for r in range(world)]
    assert np.array_equal(cat_("ranks_none"), np.concatenate(ranks))


def _sampled_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("Sampled N=")]


def test_driver_sampled_metrics_independent_of_split(tmp_path, capsys, monkeypatch):
    from tlsan_amd import train as T
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")

    def run(name, *extra):
        out = str(tmp_path / name)
        res = T.train(T.parse(["--dataset", ds, "--model_dir", out, "--max_steps", "30", "--eval_freq", "15",
                               "--eval_topk", "0"] + list(extra)))
        return res, _sampled_lines(capsys.readouterr().out), out

    res, lines, out = run("a", "--eval_negatives", "100")
    assert len(lines) == 4, lines                     # the initial, two periodic and the final evaluation
    for k in ("HR@1", "HR@10", "NDCG@10", "MRR", "AUC_N"):
        assert ("%s = " % k) in lines[0]
        assert 0.0 <= res["sampled"][k] <= 1.0
    assert res["sampled"]["HR@20"] >= res["sampled"]["HR@10"] >= res["sampled"]["HR@1"]
    tags = open(os.path.join(out, "eval", "scalars.csv")).read()
    assert ",HR@10," in tags and ",NDCG@20," in tags and ",MRR," in tags
    monkeypatch.setattr(T, "EVAL_CHUNK", 100)        # launches of 128 rows instead of 4096
    res2, lines2, _ = run("b", "--eval_negatives", "100")
    assert lines2 == lines and res2["sampled"] == res["sampled"]
    monkeypatch.setattr(T, "EVAL_CHUNK", 4096)
    res3, lines3, _ = run("c", "--eval_negatives", "100", "--test_batch_size", "32")
    assert lines3 == lines and res3["sampled"] == res["sampled"]
    # off by default: no line, no result key
    res4, lines4, _ = run("d")
    assert lines4 == [] and "sampled" not in res4

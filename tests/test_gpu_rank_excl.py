"""GPU tests of the filtered full-ranking evaluation (tlsan_eval_ranks_excl / tlsan_eval_counts_shard_excl, Model and
ShardedModel .label_ranks(exclude=, return_eligible=), the SeenItems form of `exclude`, the driver's --eval_rank_exclude):
against the fp64 oracle, exact where the candidate composition is not, list hygiene, sharded against single-GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.helpers import (batch_tuple, history_sets, host, lazy_model, make_config, model, p32, random_batch,
                           random_params)
from tests.ranks import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d,H", [(64, 8), (128, 8), (256, 8), (64, 4), (128, 16), (128, 4)])
def test_filtered_ranks_match_oracle(d, H):
    """test_eval_ranks_and_metrics' inputs, six more labels put into their own history; exclude="history".  Reference:
    the fp64 scores, counting the items ahead of the label in tf.nn.top_k's order over the items that are not excluded."""
    I = 333
    cfg = make_config(U=60, I=I, C=13, d=d, H=H)
    p = p32(random_params(cfg, seed=31))
    b, cat = random_batch(cfg, B=77, Sn=3, seed=32, test=True)
    b["hist_i"][:6, 0] = b["i"][:6]
    m = model(cfg, cat, p)
    got, elig = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude="history", return_eligible=True))
    assert got.dtype == np.int32 and elig.dtype == np.int32
    scores = orc.all_item_scores(p, cat, orc.forward(p, cat, b, H)["u_t"])
    hist = history_sets(b)
    ids = np.arange(I)
    want, want_elig, excl_ahead = np.zeros(77, np.int64), np.zeros(77, np.int64), np.zeros(77, np.int64)
    for r in range(77):
        lab = int(b["i"][r])
        out = np.isin(ids, sorted(hist[r] - {lab}))                       # the label is never excluded
        ahead = (ids != lab) & ((scores[r] > scores[r, lab]) | ((scores[r] == scores[r, lab]) & (ids < lab)))
        want[r], excl_ahead[r], want_elig[r] = (ahead & ~out).sum(), (ahead & out).sum(), I - 1 - out.sum()
    gap = np.abs(scores[np.arange(77), b["i"]][:, None] - scores)
    gap[np.arange(77), b["i"]] = np.inf
    clear = gap.min(1) > 1e-4
    print("d=%d H=%d: %d clear rows, %d with an excluded item ahead, %d labels in their own list, max |diff| %d"
          % (d, H, clear.sum(), (excl_ahead > 0).sum(), sum(int(b["i"][r]) in hist[r] for r in range(77)),
             np.abs(got - want).max()))
    assert (~clear).sum() <= 3
    assert np.array_equal(got[clear], want[clear])
    assert np.abs(got - want).max() <= 2
    assert got.min() >= 0
    assert np.array_equal(elig, want_elig)
    # not vacuous: most rows have an excluded item ahead of the label, and some labels sit in their own list
    assert (excl_ahead > 0).sum() >= 60
    assert sum(int(b["i"][r]) in hist[r] for r in range(77)) >= 6
    # the unfiltered call is untouched, and it is the filtered rank plus what was taken out
    plain = host(m.label_ranks(batch_tuple(b, True)))
    assert np.all(plain >= got) and np.array_equal((plain - got)[clear], excl_ahead[clear])


@pytest.mark.parametrize("form,table_dtype", [("dense", "f32"), ("dense", "bf16"), ("gather", "f32"), ("gather", "bf16")])
def test_exact_where_composition_is_not(form, table_dtype):
    """Lazy L2 (P != 1): the dense rank kernel fuses (acc * P) + bias, the gathering one does not, and the count of the
    listed items follows whichever ran.  With every item but the label listed the filtered rank is 0 in EVERY row (the
    composition from candidate scores is allowed 2 bad rows here: test_full_candidate_list_gives_label_rank); with
    empty lists it is label_ranks' result bit for bit."""
    I = 2000 if form == "dense" else 270000          # gather: I * d * 4 B > 256 MB
    cfg, m = lazy_model(I, table_dtype, 31)
    B = 64 if form == "dense" else 16
    b, _ = random_batch(cfg, B=B, Sn=3, seed=33, test=True)
    plain = host(m.label_ranks(batch_tuple(b, True)))
    assert plain.max() > 0
    everything = [np.arange(I)] * B                   # (the label is inside the list: it is never excluded)
    r, e = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=everything, return_eligible=True))
    assert np.array_equal(r, np.zeros(B, np.int32)), r
    assert np.array_equal(e, np.zeros(B, np.int32)), e
    r, e = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=[[]] * B, return_eligible=True))
    assert np.array_equal(r, plain) and np.all(e == I - 1)
    # half of the items: the two halves' counts add up to the whole
    lo, hi = [np.arange(I // 2)] * B, [np.arange(I // 2, I)] * B
    rl, el = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=lo, return_eligible=True))
    rh, eh = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=hi, return_eligible=True))
    assert np.array_equal((plain - rl) + (plain - rh), plain) and np.all(el + eh == I - 1)


def _raw_excl(m, batch, off, ids):
    """tlsan_eval_ranks_excl on a caller-built CSR (no cleaning on the way) -> (ranks, ahead, held)."""
    import torch
    from tlsan_amd import _lib as L
    _, _, ut, db = m.forward(batch, is_test=True, want_u_t=True)
    ws = m._workspace(db.B, db.Sn)
    out = [torch.full((db.B,), -7, dtype=torch.int32, device=m.device) for _ in range(3)]
    toff = torch.as_tensor(np.asarray(off, np.int32)).to(m.device)
    tids = torch.as_tensor(np.asarray(ids, np.int32)).to(m.device)
    L.check(m.lib.tlsan_eval_ranks_excl(C.byref(m.dims), C.byref(m.cparams), ut.data_ptr(), db.i.data_ptr(), db.B,
                                        toff.data_ptr(), tids.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                        out[2].data_ptr(), ws.data_ptr(), ws.numel(), m._stream()), "tlsan_eval_ranks_excl")
    return [host(t) for t in out]


def test_list_hygiene():
    I, B = 900, 53
    cfg = make_config(U=40, I=I, C=11, d=128)
    p = p32(random_params(cfg, seed=71))
    b, cat = random_batch(cfg, B=B, Sn=3, seed=72, test=True)
    m = model(cfg, cat, p)
    rng = np.random.RandomState(73)
    clean = [np.sort(rng.choice(I, rng.randint(1, 200), replace=False)) for _ in range(B)]
    for r in (3, 17, 52):
        clean[r] = np.zeros(0, np.int64)                                  # rows with empty lists
    clean = [c[c != b["i"][r]] for r, c in enumerate(clean)]
    want, want_e = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=clean, return_eligible=True))
    assert np.array_equal(want_e, I - 1 - np.array([len(c) for c in clean]))
    plain = host(m.label_ranks(batch_tuple(b, True)))
    assert (plain - want).sum() > 100 and (want >= 0).all()
    # repeats, ids outside the table, the label, any order, python lists
    dirty = []
    for r, c in enumerate(clean):
        x = np.concatenate([c, c[:len(c) // 2], [-1, -5, I, I + 7, 10 ** 6], [b["i"][r]] * 2]) if r % 4 else c
        dirty.append(rng.permutation(x).tolist())
    got, got_e = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=dirty, return_eligible=True))
    assert np.array_equal(got, want) and np.array_equal(got_e, want_e)
    # a row's result does not depend on the other rows' lists, nor on the rows it shares a launch with
    other = [clean[r] if r % 2 else np.arange(I) for r in range(B)]
    got = host(m.label_ranks(batch_tuple(b, True), exclude=other))
    assert np.array_equal(got[1::2], want[1::2]) and np.all(got[0::2] == 0)
    sub = {k: v[20:41] for k, v in b.items()}
    assert np.array_equal(host(m.label_ranks(batch_tuple(sub, True), exclude=clean[20:41])), want[20:41])
    # the C entry point itself on a CSR of uneven rows: ascending with repeats, ids past the table, the label
    rows = []
    for r, c in enumerate(clean):
        x = np.concatenate([c, c[::3], [b["i"][r]], [I, I + 1, 2 ** 31 - 1] if r % 3 else []]).astype(np.int64)
        rows.append(np.sort(x))
    off = np.concatenate([[0], np.cumsum([len(x) for x in rows])])
    ranks, ahead, held = _raw_excl(m, batch_tuple(b, True), off, np.concatenate(rows))
    assert np.array_equal(ranks, plain)
    assert np.array_equal(ranks - ahead, want) and np.array_equal(I - 1 - held, want_e)
    from tlsan_amd import _lib as L
    with pytest.raises(L.TlsanError, match="tlsan_eval_ranks_excl"):
        L.check(m.lib.tlsan_eval_ranks_excl(C.byref(m.dims), C.byref(m.cparams), None, None, B, None, None, None, None,
                                            None, None, 0, None), "tlsan_eval_ranks_excl")


def _seen_case(cfg, seed):
    """A synthetic train set over cfg's users and items -> (PackedSet, list of per-user sets)."""
    from tlsan_amd.input import PackedSet
    rng = np.random.RandomState(seed)
    U, I = cfg["user_count"], cfg["item_count"]
    samples = []
    for u in rng.randint(0, U - 3, 4 * U):             # (the last three users have no training sample)
        h = rng.randint(0, I, rng.randint(0, 9)).tolist()
        samples.append((int(u), h, rng.randint(0, I, rng.randint(1, 4)).tolist(), [1.0] * len(h), int(rng.randint(0, I)),
                        int(rng.randint(0, 2)), 0))
    ts = PackedSet.from_samples(samples)
    seen = [set() for _ in range(U)]
    for u, h, s, _, t, y, _ in samples:
        seen[u] |= set(h) | set(s) | ({t} if y == 1 else set())
    return ts, seen


def test_seen_form():
    from tlsan_amd.model import SeenItems
    I, B = 1200, 96
    cfg = make_config(U=50, I=I, C=11, d=64)
    p = p32(random_params(cfg, seed=81))
    b, cat = random_batch(cfg, B=B, Sn=3, seed=82, test=True)
    b["u"][:3] = [47, 48, 49]                          # users without a training sample: the row's input alone
    m = model(cfg, cat, p)
    ts, seen = _seen_case(cfg, 83)
    holder = SeenItems.from_train_set(ts, cfg["user_count"], m.device)
    assert holder.max_len == max(len(s) for s in seen)
    hist = history_sets(b)
    lists = [sorted(seen[int(b["u"][r])] | hist[r]) for r in range(B)]
    assert sum(not hist[r] <= seen[int(b["u"][r])] for r in range(B)) > B // 2      # the union matters
    got, got_e = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=holder, return_eligible=True))
    want, want_e = (host(t) for t in m.label_ranks(batch_tuple(b, True), exclude=lists, return_eligible=True))
    assert np.array_equal(got, want) and np.array_equal(got_e, want_e)
    assert np.array_equal(got_e, [I - 1 - len(set(lists[r]) - {int(b["i"][r])}) for r in range(B)])
    assert (got < host(m.label_ranks(batch_tuple(b, True), exclude="history"))).sum() > 0
    ids, _ = (host(t) for t in m.recommend(batch_tuple(b, True), 50, exclude=holder))
    for r in range(B):
        assert not set(ids[r].tolist()) & set(lists[r]), r
    # the other callers of exclusion_csr take the form as well
    neg = host(m.sample_negatives(batch_tuple(b, True), 80, exclude=holder))
    for r in range(B):
        assert not set(neg[r].tolist()) & (set(lists[r]) | {int(b["i"][r])}), r
    assert np.array_equal(host(m.sampled_ranks(batch_tuple(b, True), 80, exclude=holder)),
                          host(m.sampled_ranks(batch_tuple(b, True), 80, exclude=lists)))


def _case():
    cfg = make_config(U=61, I=1501, C=9, d=128)
    p = p32(random_params(cfg, seed=91))
    b, cat = random_batch(cfg, B=48, Sn=3, seed=92, test=True)
    b["hist_i"][:5, 0] = b["i"][:5]
    ts, seen = _seen_case(cfg, 93)
    rng = np.random.RandomState(94)
    lists = [rng.randint(-2, 1510, rng.randint(0, 300)) for _ in range(48)]      # ids outside the table among them
    return cfg, p, b, cat, ts, lists


class _Recorder:
    """Stands in for train.full_ranking_metrics: keeps the histograms it is given."""

    def __init__(self, fn):
        self.fn, self.hists = fn, []

    def __call__(self, hist, *a, **k):
        self.hists.append(np.asarray(hist, np.int64).copy())
        return self.fn(hist, *a, **k)


def _shard_worker(rank, world, out_dir):
    from tlsan_amd.dist import ShardedModel
    from tlsan_amd.model import SeenItems
    from tlsan_amd import train as T
    cfg, p, b, cat, ts, lists = _case()
    m = ShardedModel(cfg, cat, device="cuda:0")
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    holder = SeenItems.from_train_set(ts, cfg["user_count"], m.device)
    n = len(b["u"]) // world
    part = batch_tuple({k: v[rank * n:(rank + 1) * n] for k, v in b.items()}, True)
    res = {}
    for name, ex in (("history", "history"), ("seen", holder), ("lists", lists[rank * n:(rank + 1) * n])):
        r, e = m.label_ranks(part, exclude=ex, return_eligible=True)
        res["r_" + name], res["e_" + name] = host(r), host(e)
    res["plain"] = host(m.label_ranks(part))
    ids, _ = m.recommend(part, 20, exclude=holder)
    res["rec_seen"] = host(ids)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    # the drivers: no training, the full-ranking metrics of the same model over the clothing test set
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    argv = ["--dataset", ds, "--max_epochs", "0", "--quiet", "--eval_rank_exclude", "seen", "--eval_topk", "0",
            "--model_dir", os.path.join(out_dir, "r%d" % rank), "--device_input", "0"]
    rec = T.full_ranking_metrics = _Recorder(T.full_ranking_metrics)
    res = T.train_sharded(T.parse(argv + ["--sharded", "1"]))
    if rank == 0:
        h_sharded = rec.hists[-1]
        one = T.train(T.parse(argv))
        h_one = rec.hists[-1]
        assert set(res) - {"world"} == set(one) and set(res["full_ranking"]) == set(one["full_ranking"])
        assert h_sharded.sum() == h_one.sum() == 2010
        moved = int(np.abs(h_sharded - h_one).sum()) // 2
        print("rows whose filtered rank differs between the drivers: %d" % moved)
        assert moved <= 2, moved


def test_sharded_filtered_ranks_match_model(tmp_path):
    """Two processes on one GPU over gloo.  Against Model on the same launches (each rank's rows as one batch) the
    filtered ranks and the eligible counts are equal as integers; the two DRIVERS launch different batch sizes (the
    forward's u_t can differ in its last bits with the launch's batch size), so their rank histograms are
    compared with the 2-row allowance the tree's tests give near-ties."""
    from tlsan_amd.model import SeenItems
    world = 2
    run_ranks(_shard_worker, world, str(tmp_path))
    cfg, p, b, cat, ts, lists = _case()
    m = model(cfg, cat, p)
    holder = SeenItems.from_train_set(ts, cfg["user_count"], m.device)
    got = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    cat_ = lambda k: np.concatenate([g[k] for g in got])
    n = len(b["u"]) // world
    parts = [batch_tuple({k: v[r * n:(r + 1) * n] for k, v in b.items()}, True) for r in range(world)]
    for name, ex in (("history", lambda r: "history"), ("seen", lambda r: holder), ("lists", lambda r: lists[r * n:(r + 1) * n])):
        want = [m.label_ranks(parts[r], exclude=ex(r), return_eligible=True) for r in range(world)]
        assert np.array_equal(cat_("r_" + name), np.concatenate([host(w[0]) for w in want])), name
        assert np.array_equal(cat_("e_" + name), np.concatenate([host(w[1]) for w in want])), name
        assert cat_("r_" + name).dtype == np.int32 and cat_("r_" + name).min() >= 0
    assert np.array_equal(cat_("plain"), np.concatenate([host(m.label_ranks(parts[r])) for r in range(world)]))
    assert (cat_("plain") - cat_("r_seen")).sum() > 0
    rec = np.concatenate([host(m.recommend(parts[r], 20, exclude=holder)[0]) for r in range(world)])
    assert np.array_equal(cat_("rec_seen"), rec)


def _full_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith("Full ranking")]


def test_driver_full_ranking_independent_of_split(tmp_path, capsys, monkeypatch):
    from tlsan_amd import train as T
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")

    def run(name, *extra):
        out = str(tmp_path / name)
        res = T.train(T.parse(["--dataset", ds, "--model_dir", out, "--max_steps", "30", "--eval_freq", "15",
                               "--eval_topk", "0"] + list(extra)))
        return res, _full_lines(capsys.readouterr().out), out

    res, lines, out = run("a", "--eval_rank_exclude", "seen")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert len(lines) == 4, lines                     # the initial, two periodic and the final evaluation
    assert all(ln.startswith("Full ranking (exclude=seen): HR@1 = ") and " MRR = " in ln for ln in lines)
    full = res["full_ranking"]
    assert list(full) == ["HR@1", "HR@5", "HR@10", "HR@20", "NDCG@1", "NDCG@5", "NDCG@10", "NDCG@20", "MRR"]
    assert all(0.0 <= v <= 1.0 for v in full.values())
    assert full["HR@20"] >= full["HR@10"] >= full["HR@1"]
    tags = open(os.path.join(out, "eval", "scalars.csv")).read()
    assert ",Full/HR@10," in tags and ",Full/NDCG@20," in tags and ",Full/MRR," in tags
    assert ",HR@10," not in tags                      # (the sampled evaluation's tags stay its own)
    monkeypatch.setattr(T, "EVAL_CHUNK", 100)        # launches of 128 rows instead of 4096
    res2, lines2, _ = run("b", "--eval_rank_exclude", "seen")
    assert lines2 == lines and res2["full_ranking"] == full
    monkeypatch.setattr(T, "EVAL_CHUNK", 4096)
    res3, lines3, _ = run("c", "--eval_rank_exclude", "seen", "--test_batch_size", "32")
    assert lines3 == lines and res3["full_ranking"] == full
    # the other modes: fewer items kept out, the label ranks no better
    res5, lines5, _ = run("e", "--eval_rank_exclude", "none")
    res6, lines6, _ = run("f", "--eval_rank_exclude", "history")
    assert len(lines5) == len(lines6) == 4 and "(exclude=none)" in lines5[0] and "(exclude=history)" in lines6[0]
    assert full["MRR"] >= res6["full_ranking"]["MRR"] >= res5["full_ranking"]["MRR"]
    # off by default: no line, no result key, no tag
    res4, lines4, out4 = run("d")
    assert lines4 == [] and "full_ranking" not in res4
    assert "Full/" not in open(os.path.join(out4, "eval", "scalars.csv")).read()
    # 'seen' for the recommendations and the negatives
    res7, _, out7 = run("g", "--recommend_k", "10", "--recommend_exclude", "seen", "--eval_negatives", "50",
                        "--eval_neg_exclude", "seen")
    from tlsan_amd.input import load_packed, seen_items_csr
    train_set, _, (U, _, _), _ = load_packed(ds)
    off, ids = seen_items_csr(train_set, U)
    z = np.load(T.recommend_path(out7, 10))
    for r in range(0, len(z["user"]), 7):
        u = int(z["user"][r])
        assert not set(z["ids"][r].tolist()) & set(ids[off[u]:off[u + 1]].tolist()), r
    assert 0.0 <= res7["sampled"]["MRR"] <= 1.0

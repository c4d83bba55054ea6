"""GPU tests of the explanations (tlsan_explain, Model.explain): the parts against the fp64 oracle and against the kernel's
own inputs, the masks and padding bit for bit, the in-kernel selection against tests/explain_ref.select_ref over the same
call's parts, the stored forms (P != 1, bf16 tables), recommend's -1 tail, the refusals."""
import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.explain_ref import parts_ref, select_ref
from tests.helpers import batch_tuple, bits, host, lazy_model, make_config, model, p32, random_batch, random_params

pytestmark = pytest.mark.gpu

PAIRS = [(64, 8), (128, 8), (256, 8), (64, 4), (128, 16), (128, 4)]


def _items(rng, B, Kc, I, b=None, pad=0.1):
    items = rng.randint(0, I, (B, Kc))
    if b is not None:
        items[:, 0] = b["i"]
    items[rng.rand(B, Kc) < pad] = -1
    return items


def _own_bound(m, p, cat, b, H, items, got, d):
    """case 2's check: against parts_ref under the attention the kernel read, |got - ref| <= (2 d + 16) 2^-24 M per part --
    the forward-error bound of a nested dot product of that length in any summation order (each part is a sum of d, or d * d,
    products of fp32 inputs; the few elementwise roundings in front of it are the + 16)."""
    ref, M = parts_ref(p, cat, b, H, items, att0=host(m.att0), att1=host(m.att1))
    err = np.abs(got.astype(np.float64) - ref)
    bound = (2 * d + 16) * 2.0 ** -24 * M
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("explain: worst |got - ref| / bound = %.3f (max err %.3g)" % (worst, err.max()))
    assert np.all(err <= bound), worst
    return ref


@pytest.mark.parametrize("d,H", PAIRS)
def test_parts_match_oracle_and_own_inputs(d, H):
    cfg = make_config(U=60, I=700, C=13, d=d, H=H)
    p = p32(random_params(cfg, seed=11))
    b, cat = random_batch(cfg, B=77, Sn=3, seed=12, test=True)
    m = model(cfg, cat, p)
    items = _items(np.random.RandomState(13), 77, 37, 700, b)
    ex = m.explain(batch_tuple(b, True), items, top=1, parts=True)
    got = host(ex.parts)
    assert got.shape == (77, 37, 3 + 10 + 3) and got.dtype == np.float32 and tuple(ex.src.shape) == (77, 37, 1)
    # 1. against the oracle, with the oracle's own attention
    ref, _ = parts_ref(p, cat, b, H, items)
    print("explain: max |part - oracle| = %.3g" % np.abs(got - ref).max())
    assert np.abs(got - ref).max() < 1e-4
    sc = host(m.score_candidates(batch_tuple(b, True), items))
    ok = items >= 0
    assert (~ok).sum() > 100
    assert np.abs(got.astype(np.float64).sum(-1) - sc)[ok].max() < 2e-4
    # 2. against the kernel's own inputs
    _own_bound(m, p, cat, b, H, items, got, d)
    # padding items and masked positions are exactly +0.0
    assert np.all(bits(got[~ok]) == 0)
    for r in range(77):
        assert np.all(bits(got[r, :, 3 + b["sl"][r]:13]) == 0) and np.all(bits(got[r, :, 13 + b["sl_new"][r]:]) == 0)


@pytest.mark.parametrize("Ls,Sn", [(10, 3), (10, 0), (24, 2)])
def test_masks_and_padding(Ls, Sn):
    """rows with sl = 1, sl = 0 (an empty history), sl_new = 0 and sl_new = Sn; no session at all; the streamed window"""
    d, H = 64, 8
    cfg = make_config(U=40, I=300, C=9, d=d, H=H, Ls=Ls)
    p = p32(random_params(cfg, seed=21))
    b, cat = random_batch(cfg, B=37, Sn=Sn, seed=22, test=True)
    for r, n in ((0, 1), (1, 1), (2, 0)):
        b["sl"][r] = n
        b["hist_i"][r, n:] = 0
        b["hist_t"][r, n:] = 0.0
    if Sn:
        b["sl_new"][1] = 0
        b["hist_i_new"][1] = 0
        b["sl_new"][3] = Sn
        b["hist_i_new"][3] = [5, 6, 7][:Sn]
    m = model(cfg, cat, p)
    items = _items(np.random.RandomState(23), 37, 19, 300, b, pad=0.2)
    ex = m.explain(batch_tuple(b, True), items, top=4, by="position", order="abs", parts=True)
    got = host(ex.parts)
    assert got.shape == (37, 19, 3 + Ls + Sn)
    ok = items >= 0
    assert np.all(bits(got[~ok]) == 0)
    for r in range(37):
        assert np.all(bits(got[r, :, 3 + b["sl"][r]:3 + Ls]) == 0), r
        assert np.all(bits(got[r, :, 3 + Ls + b["sl_new"][r]:]) == 0), r
    assert np.all(bits(got[2, :, 3:3 + Ls]) == 0)                       # the empty history
    _own_bound(m, p, cat, b, H, items, got, d)
    sc = host(m.score_candidates(batch_tuple(b, True), items))
    assert np.abs(got.astype(np.float64).sum(-1) - sc)[ok].max() < 2e-4
    # a source is never a masked position; the empty pattern where there are fewer than 4 and for padding
    src, item, val, kind = host(ex.src), host(ex.item), host(ex.value), host(ex.kind)
    ws, wi, wv = select_ref(got, b, items, 4, "position", "abs")
    assert np.array_equal(src, ws) and np.array_equal(item, wi) and np.array_equal(bits(val), bits(wv))
    assert np.all(src[~ok] == -1) and np.all(item[~ok] == -1) and np.all(bits(val[~ok]) == 0)
    n0 = int(b["sl"][0] + b["sl_new"][0])
    assert np.all(src[0][ok[0]][:, min(n0, 4):] == -1)
    assert np.array_equal(kind, np.where(src < 0, -1, (src >= 3 + Ls).astype(np.int32)))


def _selection_case(Kc):
    cfg = make_config(U=40, I=300, C=9, d=64, H=8)
    p = p32(random_params(cfg, seed=31))
    b, cat = random_batch(cfg, B=33, Sn=3, seed=32, test=True)
    for r in range(0, 33, 3):        # the same item twice in the window and once in the session
        b["sl"][r] = max(b["sl"][r], 4)
        b["sl_new"][r] = max(b["sl_new"][r], 2)
        b["hist_i"][r, :4] = [50 + r, 60 + r, 50 + r, 70 + r]
        b["hist_t"][r, :4] = [0.5, 1.0, 0.25, 1.0 / 3]
        b["hist_i_new"][r, :2] = [80 + r, 50 + r]
    for r in (1, 4):                 # exact ties: two positions whose parts are zeros of either sign
        b["sl"][r] = max(b["sl"][r], 3)
        b["hist_i"][r, :3] = [90, 91, 92]
        b["hist_t"][r, :3] = [0.0, 0.0, 0.5]
    items = _items(np.random.RandomState(33 + Kc), 33, Kc, 300, b)
    return cfg, p, b, cat, items


@pytest.mark.parametrize("Kc", [1, 5, 17, 70])
def test_selection_matches_reference_over_own_parts(Kc):
    cfg, p, b, cat, items = _selection_case(Kc)
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    for top in (1, 3, 16):
        for by in ("item", "position"):
            for order in ("positive", "abs"):
                ex = m.explain(tup, items, top=top, by=by, order=order, parts=True)
                parts = host(ex.parts)
                ws, wi, wv = select_ref(parts, b, items, top, by, order)
                key = (Kc, top, by, order)
                assert np.array_equal(host(ex.src), ws), key
                assert np.array_equal(host(ex.item), wi), key
                assert np.array_equal(bits(host(ex.value)), bits(wv)), key
                only = m.explain(tup, items, top=top, by=by, order=order, parts=False)
                assert only.parts is None
                assert np.array_equal(host(only.src), ws) and np.array_equal(host(only.item), wi), key
                assert np.array_equal(bits(host(only.value)), bits(wv)), key
    # the case is what it claims: grouped sources differ from positions, and a tie was decided
    s_item = host(m.explain(tup, items, top=16, by="item").src)
    s_pos = host(m.explain(tup, items, top=16, by="position").src)
    assert (s_item >= 0).sum() < (s_pos >= 0).sum()
    parts = host(m.explain(tup, items, top=1, by="position", parts=True).parts)
    assert np.all(parts[1, :, 3:5] == 0.0)


def test_long_session_and_the_32_item_tile():
    """80 positions per row (a session of 70) and Kc = 20, which takes the 32-item tile: repeated items far apart, every loop
    of the kernel longer than one pass of the workgroup"""
    d, H, Sn = 128, 8, 70
    cfg = make_config(U=40, I=120, C=6, d=d, H=H)
    p = p32(random_params(cfg, seed=61))
    b, cat = random_batch(cfg, B=9, Sn=Sn, seed=62, test=True)
    b["sl_new"][:3] = [Sn, Sn - 1, 33]
    rng = np.random.RandomState(63)
    b["hist_i_new"] = np.where(np.arange(Sn)[None, :] < b["sl_new"][:, None], rng.randint(0, 120, (9, Sn)), 0)   # (120 items: repeats)
    m = model(cfg, cat, p)
    items = _items(np.random.RandomState(64), 9, 20, 120, b)
    tup = batch_tuple(b, True)
    for by, order in (("item", "positive"), ("position", "abs")):
        ex = m.explain(tup, items, top=16, by=by, order=order, parts=True)
        got = host(ex.parts)
        assert got.shape == (9, 20, 3 + 10 + Sn)
        ws, wi, wv = select_ref(got, b, items, 16, by, order)
        assert np.array_equal(host(ex.src), ws) and np.array_equal(host(ex.item), wi) and np.array_equal(bits(host(ex.value)), bits(wv))
        only = m.explain(tup, items, top=16, by=by, order=order)
        assert np.array_equal(host(only.src), ws) and np.array_equal(bits(host(only.value)), bits(wv))
    _own_bound(m, p, cat, b, H, items, got, d)
    for r in range(9):
        assert np.all(bits(got[r, :, 3 + b["sl"][r]:13]) == 0) and np.all(bits(got[r, :, 13 + b["sl_new"][r]:]) == 0)
    sc = host(m.score_candidates(tup, items))
    assert np.abs(got.astype(np.float64).sum(-1) - sc)[items >= 0].max() < 2e-4


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
def test_stored_form(table_dtype):
    """P != 1, d = 256: the parts decompose the score of the true parameters P * stored (bf16 tables widened, not rounded again)"""
    cfg, m = lazy_model(2000, table_dtype, 41)
    b, _ = random_batch(cfg, B=48, Sn=3, seed=43, test=True)
    items = _items(np.random.RandomState(44), 48, 21, 2000, b)
    tup = batch_tuple(b, True)
    ex = m.explain(tup, items, top=3, parts=True)
    got = host(ex.parts)
    P = np.float64(m.table_scale())
    assert P != 1.0
    p = {k: getattr(m, k).detach().float().cpu().numpy().astype(np.float64) * (P if k != "item_b" else 1.0)
         for k in ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb")}
    p.update({k: np.asarray(v, np.float64) for k, v in m.unpack_dense(m.dense.detach().cpu().numpy()).items()})
    cat = host(m.item_cate)
    _own_bound(m, p, cat, b, 8, items, got, 256)
    sc = host(m.score_candidates(tup, items))
    ok = items >= 0
    assert np.abs(got.astype(np.float64).sum(-1) - sc)[ok].max() < 2e-4
    ws, wi, wv = select_ref(got, b, items, 3, "item", "positive")
    assert np.array_equal(host(ex.src), ws) and np.array_equal(host(ex.item), wi) and np.array_equal(bits(host(ex.value)), bits(wv))
    assert m.table_scale() == P                      # nothing was folded


def test_with_recommend_and_refusals():
    import torch
    from tlsan_amd._lib import TlsanError
    cfg = make_config(U=40, I=300, C=9, d=128, H=8)
    p = p32(random_params(cfg, seed=51))
    b, cat = random_batch(cfg, B=29, Sn=2, seed=52, test=True)
    m = model(cfg, cat, p)
    tup = batch_tuple(b, True)
    scope = m.item_scope(items=[3, 17, 44, 101, 102, 250, 299])
    ids, sc = m.recommend(tup, 10, within=scope)
    before = {k: getattr(m, k).clone() for k in ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb", "dense", "state")}
    ex = m.explain(tup, ids, top=3, parts=True)          # a device tensor with a -1 tail
    hid = host(ids)
    assert np.all(hid[:, 7:] == -1) and np.all(hid[:, :7] >= 0)
    parts, src, item, val, kind = (host(t) for t in (ex.parts, ex.src, ex.item, ex.value, ex.kind))
    assert np.all(bits(parts[:, 7:]) == 0) and np.all(src[:, 7:] == -1) and np.all(item[:, 7:] == -1)
    assert np.all(bits(val[:, 7:]) == 0) and np.all(kind[:, 7:] == -1)
    assert np.abs(parts[:, :7].astype(np.float64).sum(-1) - host(sc)[:, :7]).max() < 2e-4
    assert np.all(src[:, :7, 0] >= 3)
    ws, wi, wv = select_ref(parts, b, hid, 3, "item", "positive")
    assert np.array_equal(src, ws) and np.array_equal(item, wi) and np.array_equal(bits(val), bits(wv))
    # refusals, all before any launch
    good = np.zeros((29, 4), np.int64)
    for bad in (np.zeros((28, 4), np.int64), np.zeros(29, np.int64), torch.zeros(29, 4, 2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            m.explain(tup, bad)
    for kw in (dict(top=0), dict(top=17), dict(top=None), dict(by="user"), dict(order="negative"), dict(top=2.5)):
        with pytest.raises(ValueError):
            m.explain(tup, good, **kw)
    over = good.copy()
    over[5, 2] = 300
    with pytest.raises(TlsanError, match="item_count"):
        m.explain(tup, over)
    # nothing in the model moved; the next list has the same bits
    for k, t in before.items():
        assert torch.equal(getattr(m, k), t), k
    ids2, sc2 = m.recommend(tup, 10, within=scope)
    assert torch.equal(ids2, ids) and np.array_equal(bits(host(sc2)), bits(host(sc)))


def test_driver_writes_explanations(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ds = os.path.join(root, "tests", "golden", "packed_clothing.npz")
    out = str(tmp_path / "model")
    r = subprocess.run([sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--max_steps", "2", "--eval_freq", "1000", "--quiet",
                        "--recommend_k", "5", "--recommend_explain", "2", "--model_dir", out],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    z = np.load(os.path.join(out, "recommend_top5.npz"))
    assert sorted(z.files) == ["ids", "scores", "user", "why_item", "why_kind", "why_value"]
    rows = len(np.load(ds)["test_u"])
    item, value, kind = z["why_item"], z["why_value"], z["why_kind"]
    assert item.shape == value.shape == kind.shape == (rows, 5, 2) and z["ids"].shape == (rows, 5)
    assert np.all(item[:, :, 0] >= 0) and np.all(np.isin(kind, (-1, 0, 1)))       # every test row has a history
    assert np.array_equal(kind < 0, item < 0) and np.all(value[item < 0] == 0)
    both = item[:, :, 1] >= 0
    assert np.all(value[:, :, 0][both] >= value[:, :, 1][both])

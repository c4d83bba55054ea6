"""CPU tests of the explanations' reference (tests/explain_ref.py) and of the Python helpers' argument checks
(tlsan_amd.model: explain_args, Explanation.columns, candidate_tensor).  The GPU side is tests/test_gpu_explain.py."""
import numpy as np
import pytest

from oracle import tlsan_oracle as orc
from tests.explain_ref import att_by_channel, parts_ref, select_ref
from tests.helpers import make_config, p32, random_batch, random_params


@pytest.mark.parametrize("d,H,Sn", [(64, 8, 3), (128, 4, 0), (64, 4, 5)])
def test_parts_sum_to_the_logit(d, H, Sn):
    cfg = make_config(U=30, I=200, C=9, d=d, H=H)
    p = p32(random_params(cfg, seed=3))
    b, cat = random_batch(cfg, B=23, Sn=Sn, seed=4, test=True)
    rng = np.random.RandomState(5)
    items = rng.randint(0, 200, (23, 6))
    items[:, 0] = b["i"]
    items[rng.rand(23, 6) < 0.15] = -1
    items[:, 0] = b["i"]
    parts, M = parts_ref(p, cat, b, H, items)
    logits = orc.forward(p, cat, b, H)["logits"]
    assert np.abs(parts[:, 0].sum(-1) - logits).max() <= 1e-12 * np.abs(logits).max()
    # every listed item's parts add up to its all-items score
    scores = orc.all_item_scores(p, cat, orc.forward(p, cat, b, H)["u_t"])
    want = np.take_along_axis(scores, np.maximum(items, 0), 1)
    ok = items >= 0
    assert np.abs(parts.sum(-1) - want)[ok].max() <= 1e-12 * np.abs(want).max()
    # masked columns, padding items
    Ls = cfg["Ls"]
    for r in range(23):
        assert np.all(parts[r, :, 3 + b["sl"][r]:3 + Ls] == 0.0) and np.all(M[r, :, 3 + b["sl"][r]:3 + Ls] == 0.0)
        assert np.all(parts[r, :, 3 + Ls + b["sl_new"][r]:] == 0.0)
    assert np.all(parts[~ok] == 0.0) and np.all(M[~ok] == 0.0)
    assert np.all(M >= np.abs(parts) * (1 - 1e-12))
    # the kernels' attention layout gives the same parts as the oracle's
    res = orc.forward(p, cat, b, H)
    lay = lambda a: a.transpose(2, 0, 1, 3).reshape(H * 23, a.shape[1], d // H)
    again, _ = parts_ref(p, cat, b, H, items, att0=lay(res["att0"]), att1=lay(res["att1"]))
    assert np.array_equal(again, parts)
    assert np.array_equal(att_by_channel(lay(res["att0"]), 23, H), res["att0"].reshape(23, Ls, d))


def _rows(hist, sl, sess, sln, parts):
    """one row, one item: the batch dict and the [1, 1, R] fp32 parts (three leading zeros for columns 0 .. 2)"""
    b = dict(hist_i=np.array([hist]), hist_i_new=np.array([sess]).reshape(1, -1), sl=np.array([sl]), sl_new=np.array([sln]))
    return b, np.array([[[0, 0, 0] + parts]], np.float32)


def _sel(b, parts, r, by, order, item=5):
    s, i, v = select_ref(parts, b, np.array([[item]]), r, by, order)
    return s[0, 0].tolist(), i[0, 0].tolist(), v[0, 0].tolist()


def test_select_ties_go_to_the_lower_column():
    b, parts = _rows([10, 11, 12, 13], 4, [14, 15], 2, [0.5, 2.0, 2.0, -2.0, 2.0, 0.5])
    assert _sel(b, parts, 4, "position", "positive") == ([4, 5, 7, 3], [11, 12, 14, 10], [2.0, 2.0, 2.0, 0.5])
    assert _sel(b, parts, 5, "position", "abs") == ([4, 5, 6, 7, 3], [11, 12, 13, 14, 10], [2.0, 2.0, -2.0, 2.0, 0.5])
    # +0.0 and -0.0 are one key
    b, parts = _rows([10, 11, 12], 3, [], 0, [-0.0, 0.0, -1.0])
    assert _sel(b, parts, 2, "position", "positive")[0] == [3, 4]
    assert _sel(b, parts, 3, "position", "abs")[0] == [5, 3, 4]


def test_select_repeated_item_across_window_and_session():
    # item 7 at columns 3, 5 (window) and 8 (session); fp32 sums in column order: (1e8 + 1) - 1e8 = 0, not 1
    b, parts = _rows([7, 9, 7, 0], 3, [8, 7], 2, [1e8, 3.0, 1.0, 99.0, 0.25, -1e8])
    for order, want in (("positive", ([4, 7, 3], [9, 8, 7], [3.0, 0.25, 0.0])), ("abs", ([4, 7, 3], [9, 8, 7], [3.0, 0.25, 0.0]))):
        assert _sel(b, parts, 3, "item", order) == want
    # by position the same row has five sources; the masked column 6 (99.0) is none
    assert _sel(b, parts, 6, "position", "positive") == ([3, 4, 5, 7, 8, -1], [7, 9, 7, 8, 7, -1], [1e8, 3.0, 1.0, 0.25, -1e8, 0.0])
    assert _sel(b, parts, 2, "position", "abs") == ([3, 8], [7, 7], [1e8, -1e8])
    # the sum keeps its sign under abs
    b, parts = _rows([7, 9, 7], 3, [], 0, [-2.0, 2.5, -1.0])
    assert _sel(b, parts, 2, "item", "abs") == ([3, 4], [7, 9], [-3.0, 2.5])
    assert _sel(b, parts, 2, "item", "positive") == ([4, 3], [9, 7], [2.5, -3.0])


def test_select_fewer_sources_than_asked_and_padding():
    b, parts = _rows([4, 5, 0, 0], 2, [0, 0], 0, [1.0, 2.0, 7.0, 7.0, 7.0, 7.0])
    for order in ("positive", "abs"):
        assert _sel(b, parts, 4, "position", order) == ([4, 3, -1, -1], [5, 4, -1, -1], [2.0, 1.0, 0.0, 0.0])
        assert _sel(b, parts, 3, "item", order) == ([4, 3, -1], [5, 4, -1], [2.0, 1.0, 0.0])
        assert _sel(b, parts, 2, "item", order, item=-1) == ([-1, -1], [-1, -1], [0.0, 0.0])


def test_select_nan_comes_last():
    b, parts = _rows([4, 5, 6], 3, [7], 1, [np.nan, -5.0, np.nan, 1.0])
    for order, first in (("positive", [6, 4]), ("abs", [4, 6])):
        s, i, v = _sel(b, parts, 4, "position", order)
        assert s == first + [3, 5] and i[2:] == [4, 6] and np.isnan(v[2]) and np.isnan(v[3])
    # a group with a NaN member is NaN
    b, parts = _rows([4, 5, 4], 3, [], 0, [1.0, -1.0, np.nan])
    s, i, v = _sel(b, parts, 2, "item", "positive")
    assert s == [4, 3] and i == [5, 4] and v[0] == -1.0 and np.isnan(v[1])


def test_python_argument_checks():
    torch = pytest.importorskip("torch")
    from tlsan_amd import _lib as L
    from tlsan_amd.model import Explanation, candidate_tensor, explain_args
    assert explain_args(3, "item", "positive") == (3, L.EXPLAIN_BY_ITEM, L.EXPLAIN_POSITIVE)
    assert explain_args(np.int64(16), "position", "abs") == (16, L.EXPLAIN_BY_POSITION, L.EXPLAIN_ABS)
    for top in (0, 17, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError):
            explain_args(top, "item", "positive")
    for by, order in (("items", "positive"), (None, "positive"), ("item", "negative"), ("item", 1)):
        with pytest.raises(ValueError):
            explain_args(3, by, order)
    assert Explanation.columns(2, 1) == ["bias", "user", "bridge", "long[0]", "long[1]", "session[0]"]
    assert len(Explanation.columns(96, 0)) == 99
    for bad in (np.zeros((4, 3), int), np.zeros(5, int), np.zeros((5, 0), int), np.zeros((5, 2, 2), int)):
        with pytest.raises(ValueError):
            candidate_tensor(bad, 5, "cpu")
    e = Explanation(None, torch.tensor([[[3, 12, 13, -1]]], dtype=torch.int32), None, None, 10)
    assert e.kind.tolist() == [[[0, 0, 1, -1]]]


def test_driver_checks_the_flag_and_writes_the_keys(tmp_path, monkeypatch):
    pytest.importorskip("torch")
    from tlsan_amd import train as T
    assert T.parse(["--dataset", "x.npz", "--recommend_k", "5"]).recommend_explain == 0
    assert T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_explain", "16"]).recommend_explain == 16
    for bad in (["--recommend_explain", "3"], ["--recommend_k", "5", "--recommend_explain", "17"],
                ["--recommend_k", "5", "--recommend_explain", "-1"], ["--recommend_k", "5", "--recommend_explain", "3", "--sharded", "1"]):
        with pytest.raises(SystemExit):
            T.parse(["--dataset", "x.npz"] + bad)
    user, ids, sc = np.arange(4), np.zeros((4, 5), np.int32), np.ones((4, 5), np.float32)
    z = np.load(T.write_recommendations(str(tmp_path), 5, user, ids, sc))
    assert sorted(z.files) == ["ids", "scores", "user"]              # without the flag: the file as it was
    why = np.zeros((4, 5, 2))
    z = np.load(T.write_recommendations(str(tmp_path), 5, user, ids, sc, why_item=why - 1, why_value=why, why_kind=why - 1))
    assert sorted(z.files) == ["ids", "scores", "user", "why_item", "why_kind", "why_value"]
    assert z["why_item"].dtype == np.int32 and z["why_value"].dtype == np.float32 and z["why_kind"].shape == (4, 5, 2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        T.parse(["--dataset", "x.npz", "--recommend_k", "5", "--recommend_explain", "3"])

"""Checks of tests/shard_ref.py itself (no GPU): the lazy owner update is the dense sweep, the element bound of
tests/test_gpu_shard_kernels.py holds for the fp32 arithmetic it is meant to allow, and bf16_rne_bits is torch's cast."""
import numpy as np
import pytest
import torch

from tests import shard_ref as sr

f32 = np.float32


def _small_problem(seed=3):
    rng = np.random.RandomState(seed)
    R, cI, Cn, G, W, ri, ru, dc = 41, 17, 5, 3, 12, 8, 11, 8
    per = [np.sort(rng.choice(R, rng.randint(6, 15), replace=False)) for _ in range(G)]
    rows = np.concatenate(per)
    src_off = np.concatenate([[0], np.cumsum([len(x) for x in per])])
    vals = rng.randn(len(rows), W)
    live = np.where(rows < cI, ri + 1, ru)
    vals[np.arange(W)[None, :] >= live[:, None]] = 0.0
    stored = rng.uniform(-0.8, 0.8, (R, W))
    cate = rng.uniform(-0.8, 0.8, (Cn, dc))
    g_cate = rng.randn(Cn, dc)
    return dict(R=R, cI=cI, G=G, W=W, ri=ri, ru=ru, rows=rows, src_off=src_off, vals=vals, stored=stored, cate=cate, g_cate=g_cate)


def test_lazy_update_is_the_dense_sweep():
    """include/tlsan.h: tlsan_shard_apply_lazy is "the same update as tlsan_shard_apply's dense sweep".  With step_dev of
    summary(P = 0.93): P_new * lazy(stored) == dense(P * stored) on the received rows, and on the others the new scale alone
    is the decay, P_new * stored == (1 - step reg) * P * stored -- in float64, to 1e-12."""
    q = _small_problem()
    P, reg, lr, G = 0.93, 1e-2, 0.05, q["G"]
    flat = np.concatenate([np.random.RandomState(1).randn(9), [0.7, 40.0, 55.0, 0.0]])
    s = sr.summary(flat, 5, 4, G, lr, reg, 0.5, 3.0, P=P)
    assert 0.05 < s["coef"] < 0.9                        # the clip bites
    sd = s["step_dev"]
    rg = np.arange(q["W"])[None, :] < sr.reg_cols(q["R"], q["cI"], q["ri"], q["ru"])[:, None]
    args = (q["rows"], q["src_off"], q["vals"], q["g_cate"], q["cI"], q["W"], q["ri"], q["ru"], 1.0 / G)
    lw, lc, P_new, _, _ = sr.apply_lazy(q["stored"], q["cate"], *args, sd)
    true0 = np.where(rg, P * q["stored"], q["stored"])          # (item_b and the padding are not scaled)
    dw, dc_, _, _ = sr.apply_dense(true0, P * q["cate"], *args, s["step"], s["coef"], reg)
    assert P_new == sd[3]
    got = np.zeros(q["R"], bool)
    got[q["rows"]] = True
    assert got.any() and not got.all()
    true1 = np.where(rg, P_new * lw, lw)
    scale = np.abs(dw).max()
    assert np.abs(true1 - dw)[got].max() <= 1e-12 * scale
    assert np.abs(P_new * lc - dc_).max() <= 1e-12 * np.abs(dc_).max()
    # rows nobody sent: stored bits stay, the scale carries the decay (regularised columns; the others do not move at all)
    assert np.array_equal(lw[~got], q["stored"][~got])
    rest = (P_new * q["stored"] - (1.0 - s["step"] * reg) * P * q["stored"])[~got]
    assert np.abs(rest).max() <= 1e-12 * scale
    assert np.abs((true1 - dw)[~got][rg[~got]]).max() <= 1e-12 * scale
    assert np.array_equal(dw[~got][~rg[~got]], q["stored"][~got][~rg[~got]])


def test_lazy_sums_of_squares():
    q = _small_problem(4)
    G = q["G"]
    sd = [0.02, 0.4, 0.0215, 0.93]
    lw, lc, _, d0, s1 = sr.apply_lazy(q["stored"], q["cate"], q["rows"], q["src_off"], q["vals"], q["g_cate"], q["cI"], q["W"],
                                      q["ri"], q["ru"], 1.0 / G, sd)
    rg = np.arange(q["W"])[None, :] < sr.reg_cols(q["R"], q["cI"], q["ri"], q["ru"])[:, None]
    assert abs(d0 - ((lw ** 2)[rg].sum() - (q["stored"] ** 2)[rg].sum())) < 1e-12
    assert abs(s1 - (lc ** 2).sum()) < 1e-12


@pytest.mark.parametrize("G", [1, 3, 5, 16])
def test_element_bound_holds_for_fp32_arithmetic(G):
    """The dense SGD element update and the lazy one emulated in fp32 -- the source sum exact (the kernels add in double),
    then every product and sum rounded on its own, or every multiply-add rounded once (what a compiler that contracts
    makes of it) -- against the float64 reference: |error| <= 8 * 2^-24 * S with the S of tests/test_gpu_shard_kernels.py."""
    rng = np.random.RandomState(G)
    n = 400_000
    w0 = rng.uniform(-0.8, 0.8, n).astype(f32)
    nsrc = rng.randint(0, G + 1, n)                                        # sources that sent the element's row
    v = rng.randn(G, n).astype(f32) * (np.arange(G)[:, None] < nsrc[None, :])
    sig = v.astype(np.float64).sum(0)                                      # (G <= 16 fp32 values: exact in double)
    gscale, reg, step, lazy = f32(1.0 / G), f32(1e-2), f32(0.05 * 0.37), f32(0.05 * 0.37 / 0.92)
    d = np.float64
    r32 = lambda x: np.asarray(x, np.float64).astype(f32)                  # one rounding of an exactly known value
    sf = r32(sig)
    # ---- dense: w - step * (gscale * sum + reg * w)
    ref = d(w0) - d(step) * (d(gscale) * sig + d(reg) * d(w0))
    S = np.abs(d(w0)) + d(step) * (d(gscale) * np.abs(sig) + d(reg) * np.abs(d(w0)))
    g_sep = (gscale * sf) + (reg * w0)                                     # fp32 operators: each rounds
    sep = w0 - step * g_sep
    g_fma = r32(d(gscale) * d(sf) + d(reg * w0))
    fma = r32(d(w0) - d(step) * d(g_fma))
    for name, got in (("separate", sep), ("contracted", fma)):
        assert got.dtype == f32
        worst = (np.abs(d(got) - ref) / (sr.U32 * S)).max()
        assert worst <= 8.0, ("dense", name, worst)
    # ---- lazy: w - s * (gscale * sum)
    ref = d(w0) - d(lazy) * (d(gscale) * sig)
    S = np.abs(d(w0)) + d(lazy) * d(gscale) * np.abs(sig)
    t = gscale * sf
    sep = w0 - lazy * t
    fma = r32(d(w0) - d(lazy) * d(t))
    for name, got in (("separate", sep), ("contracted", fma)):
        assert got.dtype == f32
        worst = (np.abs(d(got) - ref) / (sr.U32 * S)).max()
        assert worst <= 8.0, ("lazy", name, worst)


def test_bf16_rne_bits_is_torchs_cast():
    rng = np.random.RandomState(0)
    x = rng.randn(1_000_000).astype(f32)
    planted = np.array([b for b, _ in sr.BF16_PLANTED], np.uint32).view(f32)
    x[:len(planted)] = planted
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = sr.bf16_rne_bits(x)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert got[:len(planted)].tolist() == [h for _, h in sr.BF16_PLANTED]


def test_summary_reference_by_hand():
    """two dense gradients, G = 2, no clipping: the numbers of the issue's formulas worked out by hand"""
    flat = np.array([0.6, -0.8, 9.0, 1.4, 8.0, 5.0])          # dense | cate | BCE, row squares, table squares
    s = sr.summary(flat, 2, 1, 2, 0.5, 0.1, 10.0, 3.0, P=0.5, dense=np.array([1.0, 2.0]))
    S_tot = (5.0 + 3.0) * 0.25
    norm = np.sqrt(8.0 / 4 + 0.01 * S_tot + 0.09 + 0.16)
    assert abs(s["norm"] - norm) < 1e-15 and s["coef"] == 1.0 and s["step"] == 0.5
    assert abs(s["loss"] - (0.7 + 0.05 * S_tot)) < 1e-15
    P_new = 0.5 * (1 - 0.05)
    assert np.allclose(s["step_dev"], [0.5, 1.0, 0.5 / P_new, P_new], rtol=1e-15)
    assert np.allclose(s["dense"], [1.0 - 0.15, 2.0 + 0.2], rtol=1e-15)
    c = sr.summary(flat, 2, 1, 2, 0.5, 0.1, 0.3, 3.0)
    assert c["S_tot"] == 8.0 and abs(c["norm"] - np.sqrt(2.0 + 0.08 + 0.25)) < 1e-15      # (no scale: P = 1)
    assert abs(c["coef"] - 0.3 / c["norm"]) < 1e-15 and len(c["step_dev"]) == 2

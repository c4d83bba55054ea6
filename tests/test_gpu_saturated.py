"""GPU tests of the fused kernels' softmaxes under peaked, saturated and tied attention, and of the loss term under
large logits: the inputs of tests/saturated.py (family A `sharpened`, family B `planted`; tests/test_saturated_cpu.py
asserts that they are as extreme as this file needs), every output of the kernels against the fp64 oracle on the
fp32-rounded parameters with the same number of heads.

Tolerances: per compared quantity the one the suite already uses for it (1e-4 logits and u_t, 2e-5 attention weights,
2e-4 -- streamed windows 3e-4 -- of the largest entry for gradients, norms and updates, with the suite's absolute
floors), or 4 x the error of the oracle itself run in fp32 on the same inputs where that is larger (saturated.tol).
Every comparison prints `RATIO <case> <quantity> <kernel error> <fp32-oracle error> <their ratio>` before it asserts;
profiles/saturated_attention.md keeps the ratios measured on an MI355X.

Out of scope: bf16 MATRIX operands -- a 2^-8 relative error on a score of 50 log2 units moves weights by tens of
percent, so no meaningful bound exists at this sharpness (bf16 TABLES are exact inputs and are tested) -- and the
sharded drivers, which run these same kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import saturated as sat
from tests.helpers import BF16_TABLES, batch_tuple, bf16_round, model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("A", s) for s in sat.SHAPES] + [("B", s) for s in sat.SHAPES_B]
IDS = ["%s-%s" % (f, sat.case_id(s)) for f, s in CASES]


def _cmp(case, what, err, bound, e32):
    """print the kernel's error beside the fp32 oracle's, then hold it to the bound"""
    print("RATIO %s %s %.3e %.3e %.2f" % (case, what, err, e32, err / e32 if e32 > 0 else 0.0))
    assert err < bound, (case, what, err, bound, e32)


def _rel(streamed):
    return 3e-4 if streamed else 2e-4


def _half_ulp(x):
    """half an ulp of the largest fp32 entry: what storing p - lr * g in fp32 may move an update `new - old` by (the
    suite's floors of 2e-7 .. 5e-7 cover parameters up to about 4; a sharpened W2 reaches 60)"""
    return 0.5 * float(np.spacing(np.float32(np.abs(x).max())))


def _check_grads(cid, out, ref, rel, e32=None):
    e32 = ref["e32"] if e32 is None else e32
    for k, g in ref["g"].items():
        gk = np.asarray(out["grads"][k], np.float64).reshape(g.shape)
        assert np.isfinite(gk).all(), k
        gmax = float(np.abs(g).max())
        _cmp(cid, "grad/" + k, float(np.abs(gk - g).max()), max(rel * gmax, 4.0 * e32["g"][k]) + 1e-6, e32["g"][k])


def _check_step(cid, m, loss, c, ref, tag, rel_loss, rel_norm, rel, floor):
    """loss, last_gnorm() and every parameter's update new - old against the oracle's step, at the suite's tolerances for
    the kind of step (rel_loss of max(1, |loss|), rel_norm of the norm, rel of the largest update + floor)"""
    e = ref["e32"]
    assert np.isfinite(loss)
    _cmp(cid, tag + "/loss", abs(loss - ref["loss"]), sat.tol(rel_loss * max(1.0, abs(ref["loss"])), e["loss"]), e["loss"])
    _cmp(cid, tag + "/gnorm", abs(m.last_gnorm() - ref["n18"]) / ref["n18"], sat.tol(rel_norm, e["n18"]), e["n18"])
    got = m.get_params()
    for k, new in ref["newp"].items():          # (the form of test_gpu_heads._check_update)
        a = np.asarray(got[k], np.float64).reshape(new.shape)
        assert np.isfinite(a).all(), k
        du, dr = a - c["p"][k], new - c["p"][k]
        bound = max(rel * (np.abs(dr).max() + 1e-9), 4.0 * e["upd"][k]) + max(floor, _half_ulp(new))
        _cmp(cid, tag + "/upd/" + k, float(np.abs(du - dr).max()), bound, e["upd"][k])


@pytest.mark.parametrize("family,shape", CASES, ids=IDS)
def test_forward_logits_and_u_t(family, shape):
    c = sat.case(family, shape)
    cid, ref, e = "%s-%s" % (family, sat.case_id(shape)), c["ref"], c["ref"]["e32"]
    m = model(c["cfg"], c["cat"], c["p"])
    li, lj, ut, _ = m.forward(batch_tuple(c["b"], True), is_test=True, want_u_t=True)
    li, lj, ut = li.cpu().numpy(), lj.cpu().numpy(), ut.cpu().numpy()
    assert np.isfinite(li).all() and np.isfinite(lj).all() and np.isfinite(ut).all()
    _cmp(cid, "logits", float(np.abs(li - ref["fwd"]["logits"]).max()), sat.tol(1e-4, e["logits"]), e["logits"])
    _cmp(cid, "logits_j", float(np.abs(lj - ref["fwd_j"]["logits"]).max()), sat.tol(1e-4, e["logits_j"]), e["logits_j"])
    _cmp(cid, "u_t", float(np.abs(ut - ref["fwd"]["u_t"]).max()), sat.tol(1e-4, e["u_t"]), e["u_t"])
    lt, _, _, _ = m.forward(batch_tuple(c["b"]), is_test=False)
    lt = lt.cpu().numpy()
    assert np.isfinite(lt).all()
    _cmp(cid, "logits_train", float(np.abs(lt - ref["fwd"]["logits"]).max()), sat.tol(1e-4, e["logits"]), e["logits"])


@pytest.mark.parametrize("family,shape", CASES, ids=IDS)
def test_attention_weights(family, shape):
    d, H, Ls, Sn = shape
    c = sat.case(family, shape)
    cid, ref, e, b = "%s-%s" % (family, sat.case_id(shape)), c["ref"], c["ref"]["e32"], c["b"]
    B = len(b["u"])
    m = model(c["cfg"], c["cat"], c["p"])
    m.forward(batch_tuple(b, True), is_test=True, want_att=True)
    scores = sat.planted_scores(c["p"], c["cat"], b, H)[:2] if family == "B" else (None, None)
    blocks = (("att0", m.att0, ref["fwd"]["att0"], Ls, b["sl"], scores[0], "long"),
              ("att1", m.att1, ref["fwd"]["att1"], Sn + 1, b["sl_new"] + 1, scores[1], "short"))
    for name, got, want, T, length, sc, blk in blocks:
        g = got.cpu().numpy()
        w = sat.att_rows(want, H)
        assert g.shape == w.shape and np.isfinite(g).all()
        _cmp(cid, name, float(np.abs(g - w).max()), sat.tol(2e-5, e[name]), e[name])
        masked = np.arange(T)[None, :] >= np.tile(np.asarray(length), H)[:, None]
        assert (g[masked] == 0.0).all()
        assert np.abs(g.sum(1) - 1.0).max() < 1e-5
        if family != "B":
            continue
        gb = g.reshape(H, B, T, d // H).transpose(1, 2, 0, 3).reshape(B, T, d)     # back to [sample, position, channel]
        for r, pl in enumerate(c["info"][blk]):
            n = int(length[r])
            if pl["profile"] == "tie_all":       # an exact tie of all valid positions: 1 / n each
                assert np.abs(gb[r, :n] - 1.0 / n).max() < sat.tol(2e-5, e[name]), (name, r, n)
            elif pl["profile"] == "tie_two" and n > 2:     # an exact tie of two peaks: the same weight for both
                top = np.argsort(sc[r, :n], axis=0)[-2:]
                tied = np.take_along_axis(sc[r, :n], top, 0)
                ch = np.nonzero(tied[0] == tied[1])[0]
                assert len(ch) >= d // 4
                assert np.abs(gb[r, top[0][ch], ch] - gb[r, top[1][ch], ch]).max() < sat.tol(2e-5, e[name]), (name, r)
            elif pl["profile"] == "cliff":       # more than 130 log2 units below the peak: exactly 0 in fp32
                far = (sc[r, :n].max(axis=0)[None, :] - sc[r, :n]) / np.log(2.0) > 130.0
                assert far.any() and (gb[r, :n][far] == 0.0).all(), (name, r)


@pytest.mark.parametrize("family,shape", CASES, ids=IDS)
def test_gradients_both_norm_modes(family, shape):
    c = sat.case(family, shape)
    cid, ref, e = "%s-%s" % (family, sat.case_id(shape)), c["ref"], c["ref"]["e32"]
    streamed = shape[2] > 10
    out = model(c["cfg"], c["cat"], c["p"]).grads(batch_tuple(c["b"]))
    assert np.isfinite(out["logits"]).all() and np.isfinite(out["loss"]) and np.isfinite(out["gnorm"])
    _cmp(cid, "grads/logits", float(np.abs(out["logits"] - ref["logits"]).max()), sat.tol(1e-4, e["logits"]), e["logits"])
    _cmp(cid, "grads/loss", abs(out["loss"] - ref["loss"]), sat.tol(1e-4 * max(1.0, abs(ref["loss"])), e["loss"]), e["loss"])
    _check_grads(cid, out, ref, _rel(streamed))
    _cmp(cid, "gnorm/tf18", abs(out["gnorm"] - ref["n18"]) / ref["n18"], sat.tol(_rel(streamed), e["n18"]), e["n18"])
    out2 = model(c["cfg"], c["cat"], c["p"], norm_mode="dedup").grads(batch_tuple(c["b"]))
    _cmp(cid, "gnorm/dedup", abs(out2["gnorm"] - ref["nd"]) / ref["nd"], sat.tol(_rel(streamed), e["nd"]), e["nd"])


@pytest.mark.parametrize("l2_mode", ["dense", "lazy"])
@pytest.mark.parametrize("family,shape", CASES, ids=IDS)
def test_train_step(family, shape, l2_mode):
    c = sat.case(family, shape)
    cid = "%s-%s" % (family, sat.case_id(shape))
    streamed = shape[2] > 10
    m = model(c["cfg"], c["cat"], c["p"], l2_mode=l2_mode)
    loss = m.train(None, batch_tuple(c["b"]), sat.LR)
    if streamed:      # (test_long_windows_streamed's tolerances; test_train_step_matches_oracle's)
        _check_step(cid, m, loss, c, c["ref"], "train-" + l2_mode, 2e-4, 3e-4, 3e-4, 5e-7)
    else:
        _check_step(cid, m, loss, c, c["ref"], "train-" + l2_mode, 1e-4, 2e-4, 2e-4, 2e-7)


def test_bf16_tables():
    """bf16 table storage at a streamed, sharpened case: the oracle runs on the bf16-rounded tables (exact inputs to
    both), as in test_bf16_tables_with_streamed_windows."""
    shape = (128, 8, 33, 3)
    c = sat.case("A", shape)
    p = dict(c["p"])
    for k in BF16_TABLES:
        p[k] = bf16_round(p[k]).astype(np.float64)
    ref = sat.reference(p, c["cat"], c["b"], c["H"], c["cfg"]["regulation_rate"])
    e = ref["e32"]
    m = model(c["cfg"], c["cat"], p, l2_mode="lazy", table_dtype="bf16")
    li, _, _, _ = m.forward(batch_tuple(c["b"]), is_test=False)
    li = li.cpu().numpy()
    assert np.isfinite(li).all()
    _cmp("bf16-tables", "logits", float(np.abs(li - ref["fwd"]["logits"]).max()), sat.tol(1e-4, e["logits"]), e["logits"])
    out = m.grads(batch_tuple(c["b"]))
    _check_grads("bf16-tables", out, ref, 3e-4)
    loss = model(c["cfg"], c["cat"], p, l2_mode="lazy", table_dtype="bf16").train(None, batch_tuple(c["b"]), sat.LR)
    _cmp("bf16-tables", "loss", abs(loss - ref["loss"]), sat.tol(2e-4 * max(1.0, abs(ref["loss"])), e["loss"]), e["loss"])


@pytest.mark.parametrize("shape", [(128, 8, 10, 4), (128, 8, 33, 3)], ids=sat.case_id)
def test_dropout(shape):
    """dropout at rate 0.3 on sharpened scores: the step follows the oracle's under the kernel's own keep pattern (with
    streamed windows dropout keeps one window per column group, the online softmax without the flat work list)."""
    rate = 0.3
    c = sat.case("A", shape)
    cid = "dropout-" + sat.case_id(shape)
    cfg = dict(c["cfg"], dropout=rate)
    m = model(cfg, c["cat"], c["p"])
    seed = m.dropout_seed()
    ref = sat.reference(c["p"], c["cat"], c["b"], c["H"], cfg["regulation_rate"], dropout=(rate, seed))
    assert abs(ref["loss"] - c["ref"]["loss"]) > 1e-5          # (the pattern changes the step)
    loss = m.train(None, batch_tuple(c["b"]), sat.LR)
    _check_step(cid, m, loss, c, ref, "train", 1e-4, 2e-4, 3e-4, 3e-7)    # (test_dropout_training_matches_oracle's tolerances)


@pytest.mark.parametrize("shape", [sat.SHAPES[0], sat.SHAPES[1]], ids=sat.case_id)
def test_large_logits(shape):
    """Logits of +-20, +-60 and +-100 under both labels: the loss term's exp(-|x|), log(1 + e) and fast reciprocal at
    their ends -- a sigmoid that equals the label in fp32, a loss of 100 for one sample."""
    c = sat.case("A", shape)
    cid = "logits-" + sat.case_id(shape)
    p, b, want = sat.plant_logits(c["p"], c["cat"], c["b"], c["H"])
    ref = sat.reference(p, c["cat"], b, c["H"], c["cfg"]["regulation_rate"])
    e = ref["e32"]
    assert np.abs(ref["logits"][:len(want)] - want).max() < 1e-4
    out = model(c["cfg"], c["cat"], p).grads(batch_tuple(b))
    assert np.isfinite(out["logits"]).all() and np.isfinite(out["loss"]) and np.isfinite(out["gnorm"])
    _cmp(cid, "grads/loss", abs(out["loss"] - ref["loss"]), 1e-4 * max(1.0, abs(ref["loss"])), e["loss"])
    _check_grads(cid, out, ref, 2e-4)
    _cmp(cid, "gnorm/tf18", abs(out["gnorm"] - ref["n18"]) / ref["n18"], 2e-4, e["n18"])
    m = model(c["cfg"], c["cat"], p)
    loss = m.train(None, batch_tuple(b), sat.LR)
    assert np.isfinite(loss)
    _cmp(cid, "train/loss", abs(loss - ref["loss"]), 1e-4 * max(1.0, abs(ref["loss"])), e["loss"])
    _cmp(cid, "train/gnorm", abs(m.last_gnorm() - ref["n18"]) / ref["n18"], 2e-4, e["n18"])
    got = m.get_params()
    for k in got:
        assert np.isfinite(np.asarray(got[k])).all(), k
    du = np.asarray(got["item_b"], np.float64).reshape(p["item_b"].shape) - p["item_b"]
    dr = ref["newp"]["item_b"] - p["item_b"]
    _cmp(cid, "train/upd/item_b", float(np.abs(du - dr).max()), 2e-4 * (np.abs(dr).max() + 1e-9) + max(2e-7, _half_ulp(p["item_b"])),
         e["upd"]["item_b"])


N_D128 = sum(1 for _, s in CASES if s[0] == 128) * 5 + 1 + 2 + 1   # forward, attention, gradients, two steps; bf16; dropout; logits


def test_d128_cases_in_the_16_sample_geometry():
    """d = 128 launches of up to 1024 sequences take the 8-sample workgroups, so the batches of this file never reach the
    16-sample kernel the bench shape runs: every d = 128 case again in a child process under TLSAN_NW4=0 (read once per
    process), as test_d128_parity_in_both_workgroup_geometries does."""
    env = dict(os.environ, TLSAN_NW4="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_saturated.py", "-m", "gpu", "-q", "-x", "-k",
                        "(d128 or bf16) and not geometry"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    mt = re.search(r"(\d+) passed", r.stdout)
    assert mt and int(mt.group(1)) >= N_D128, r.stdout[-2000:]

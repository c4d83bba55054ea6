"""The saturated-attention inputs of tests/saturated.py against the fp64 oracle alone: the planted scores are what the
construction says, every case is as peaked as tests/test_gpu_saturated.py needs it to be (so that test cannot pass
vacuously), and the fp32 oracle's own error -- which sets the GPU tolerances -- stays below the caps.  No GPU."""
import numpy as np
import pytest

from tests import saturated as sat

CASES = [("A", s) for s in sat.SHAPES] + [("B", s) for s in sat.SHAPES_B]
IDS = ["%s-%s" % (f, sat.case_id(s)) for f, s in CASES]
TINY = 2.0 ** -126


def _blocks(c):
    """(name, oracle weights [B, T, d], lengths) of the long and the short block"""
    b, f = c["b"], c["ref"]["fwd"]
    B = len(b["u"])
    return (("long", f["att0"].reshape(B, f["att0"].shape[1], -1), b["sl"]),
            ("short", f["att1"].reshape(B, f["att1"].shape[1], -1), b["sl_new"] + 1))


@pytest.mark.parametrize("shape", sat.SHAPES_B, ids=sat.case_id)
def test_planted_attention_is_the_closed_form(shape):
    c = sat.case("B", shape)
    s0, s1, zmin = sat.planted_scores(c["p"], c["cat"], c["b"], c["H"])
    assert zmin > 0.05, "a relu is closed (or nearly): the scores are not linear in the input"
    for (name, att, length), sc in zip(_blocks(c), (s0, s1)):
        assert np.abs(att - sat.masked_softmax(sc, length)).max() < 1e-12, name
    assert (c["b"]["sl"] < shape[2]).any() and (c["b"]["sl_new"] < shape[3]).any()


@pytest.mark.parametrize("family,shape", CASES, ids=IDS)
def test_half_of_the_softmaxes_are_peaked(family, shape):
    for name, att, _ in _blocks(sat.case(family, shape)):
        frac = float((att.max(axis=1) > 0.9).mean())
        print("%s %s %s: largest weight > 0.9 in %.3f of the softmaxes" % (family, sat.case_id(shape), name, frac))
        assert frac >= 0.5, (name, frac)


@pytest.mark.parametrize("family,shape", [c for c in CASES if c[1][2] > 10], ids=[i for i, c in zip(IDS, CASES) if c[1][2] > 10])
def test_streamed_windows_hold_weights_that_underflow_fp32(family, shape):
    name, att, length = _blocks(sat.case(family, shape))[0]
    valid = np.arange(att.shape[1])[None, :] < length[:, None]
    frac = float((att[valid] < TINY).mean())
    print("%s %s: %.4f of the valid window weights below 2^-126" % (family, sat.case_id(shape), frac))
    assert frac >= 0.01


def _placed(att, rows, pos):
    """(sample, channel) softmaxes of samples `rows` whose weight at position pos[row] exceeds 0.999"""
    return int(sum((att[r, pos[r]] > 0.999).sum() for r in rows))


@pytest.mark.parametrize("shape", sat.SHAPES_B, ids=sat.case_id)
def test_planted_peak_placements_are_realised(shape):
    d, H, Ls, Sn = shape
    c = sat.case("B", shape)
    nlc, nl = sat.chunk_lengths(d, H)
    assert nlc in (16, 32) and nl in (16, 32)
    for (name, att, length), n_max in zip(_blocks(c), (Ls, Sn + 1)):
        rows = np.arange(att.shape[0])
        multi = [r for r in rows if length[r] > 1]
        want = {"first": np.zeros(len(rows), int), "last valid": length - 1}
        # the last position of a chunk and the first of the next: the kernel's own chunk length and every other multiple
        # of 16 that fits (short block: session entry k is position k + 1)
        off = 0 if name == "long" else 1
        ks = [k for k in range(16, n_max - off, 16)]
        if name == "long" and Ls > 10:
            assert nlc in ks
        if name == "short" and Sn > 16:
            assert 16 in ks and (nl in ks or nl + off >= n_max)
        for k in ks:
            want["chunk end %d" % k] = np.full(len(rows), k - 1 + off)
            want["chunk start %d" % k] = np.full(len(rows), k + off)
        for what, pos in want.items():
            ok = [r for r in multi if pos[r] < length[r]]
            n = _placed(att, ok, pos)
            print("%s %s: peak at %s in %d softmaxes" % (sat.case_id(shape), name, what, n))
            assert n >= 32, (name, what, n)


@pytest.mark.parametrize("shape", sat.SHAPES_B, ids=sat.case_id)
def test_planted_ties_cliffs_monotone_runs_and_zero_inputs(shape):
    c = sat.case("B", shape)
    b, info = c["b"], c["info"]
    scores = sat.planted_scores(c["p"], c["cat"], b, c["H"])[:2]
    for (name, att, length), sc, plans in zip(_blocks(c), scores, (info["long"], info["short"])):
        seen = set()
        for r, pl in enumerate(plans):
            n = int(length[r])
            assert pl["n"] == n
            s, a = sc[r, :n], att[r, :n]
            seen.add(pl["profile"])
            if pl["profile"] == "tie_all":
                assert n > 1 and np.abs(a - 1.0 / n).max() < 1e-12
            elif pl["profile"] == "tie_two" and n > 2:
                top = np.sort(s, axis=0)[-2:]
                up = top[1] == top[0]                       # (channels whose largest level is the tied one)
                assert up.sum() >= a.shape[1] // 4 and np.abs(np.sort(a, axis=0)[-1][up] - 0.5).max() < 1e-4
            elif pl["profile"] == "cliff" and n > 1:
                gap = (s.max(axis=0)[None, :] - s) / np.log(2.0)
                far = gap > 0
                assert (gap[far] > 130.0).all() and (a[far] < 2.0 ** -130).all()
                assert (far.sum(axis=0) == n - 1).sum() >= a.shape[1] // 4      # a lone peak over n - 1 far positions
            elif pl["profile"] in ("rise", "fall") and n > 2:
                step = np.diff(s, axis=0)
                always = (step > 0).all(axis=0).mean()      # the running maximum is replaced at every position
                never = (step < 0).all(axis=0).mean()       # ... at none after the first
                assert always >= 0.25 and never >= 0.25, (name, always, never)
                seen.add(pl["profile"] + "+")
        assert {"tie_all", "tie_two", "cliff", "rise+", "fall+", "peak"} <= seen, (name, seen)
    zero = [(r, pl["zero"]) for r, pl in enumerate(info["long"]) if pl["zero"] is not None]
    assert zero and all(b["hist_t"][r, z] == 0.0 and z < b["sl"][r] for r, z in zero)


@pytest.mark.parametrize("family,shape", CASES, ids=IDS)
def test_fp32_oracle_error_stays_below_the_caps(family, shape):
    """What an fp32 run of the oracle itself loses on every compared quantity: a case beyond these caps is too sharp to
    be a test of fp32 kernels."""
    ref = sat.case(family, shape)["ref"]
    e = ref["e32"]
    print("%s %s fp32 oracle error: " % (family, sat.case_id(shape)) +
          " ".join("%s %.2e" % (k, e[k]) for k in ("logits", "logits_j", "u_t", "att0", "att1", "loss", "n18", "nd")))
    for k in ("logits", "logits_j", "u_t", "att0", "att1"):
        assert e[k] < 1e-4, (k, e[k])
    assert e["loss"] < 1e-4 * max(1.0, abs(ref["loss"]))
    assert e["n18"] < 2e-4 and e["nd"] < 2e-4
    for k, g in ref["g"].items():
        gmax = float(np.abs(g).max())
        print("    grad %-10s largest %.3e  fp32 error %.2e (%.2e of it)" % (k, gmax, e["g"][k], e["g"][k] / (gmax + 1e-300)))
        assert e["g"][k] < 2e-4 * gmax + 1e-6, (k, e["g"][k], gmax)
        assert np.isfinite(g).all()


@pytest.mark.parametrize("shape", [sat.SHAPES[0], sat.SHAPES[1]], ids=sat.case_id)
def test_planted_logits_reach_their_targets(shape):
    from oracle import tlsan_oracle as orc
    c = sat.case("A", shape)
    p, b, want = sat.plant_logits(c["p"], c["cat"], c["b"], c["H"])
    logits = orc.forward(p, c["cat"], b, c["H"])["logits"]
    n = len(want)
    assert np.abs(logits[:n] - want).max() < 1e-4          # (item_b is rounded to fp32: half an ulp of 100 is 4e-6)
    got = set(zip(np.sign(want).astype(int).tolist(), np.abs(want).astype(int).tolist(), b["y"][:n].astype(int).tolist()))
    assert got == {(s, m, y) for s in (1, -1) for m in (20, 60, 100) for y in (0, 1)}
    ref = sat.reference(p, c["cat"], b, c["H"], c["cfg"]["regulation_rate"])
    e = ref["e32"]
    print("%s planted logits: loss %.4f, fp32 oracle error loss %.2e item_b %.2e n18 %.2e"
          % (sat.case_id(shape), ref["loss"], e["loss"], e["g"]["item_b"], e["n18"]))
    assert e["loss"] < 1e-4 * max(1.0, abs(ref["loss"])) and e["n18"] < 2e-4
    assert e["g"]["item_b"] < 2e-4 * np.abs(ref["g"]["item_b"]).max() + 1e-6

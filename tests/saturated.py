"""Inputs with peaked, saturated and tied attention for the softmaxes of the fused kernels (tlsan_attn.h), and the cases
tests/test_saturated_cpu.py (the inputs themselves, against the fp64 oracle) and tests/test_gpu_saturated.py (the kernels)
share.  Importable without a GPU.

Family A, `sharpened`: tests.helpers.random_params with fwa1_W2 / fwa2_W2 multiplied by a sharpness S -- the dense
random MLP and its relu kinks stay, the scores grow S-fold.

Family B, `planted`: every score is an explicit linear function of the position.  With W1 = c I, b1 = beta (every relu
open), W2 = kappa I the score of channel ch at position t is kappa (c x[t, ch] + beta) + b2[ch].  All table rows are a
scalar LEVEL times one sign / magnitude pattern sigma (|sigma| in [0.6, 0.8], half of the channels of either sign), so
x[t, ch] = sigma[ch] * level[t] and the softmax of channel ch is softmax_t(alpha[ch] * level[t]) with
alpha = kappa c sigma: channels with alpha > 0 peak where the level is largest, channels with alpha < 0 where it is
smallest.  A profile therefore names a PEAK position (largest level) and an ANTI-PEAK position (smallest level), and
each placement is realised in half of the channels by either.
  long block: every valid position of a sample holds the same item (level +1 or -1); the level of position t is
    s_t = gamma * usert_emb[u, t] * hist_t[t], written through the user's usert_emb row (one user per sample).
  short block: dense_K = 0, so the bridge (position 0) is exactly dense_b = MID * sigma; session position t holds an item
    (and its category) of the wanted level.
Levels: peaks stand A_M above (anti-peaks below) the other positions, which differ among themselves by a ramp of at
most RAMP: a gap of at least KC * 0.6 * (A_M - RAMP) = 13.3 nats, weight > 0.999 among 90 positions.  A cliff stands A_C
above: at least KC * 0.6 * A_C = 93.6 nats = 135 log2 units, past the 126 at which exp2 underflows to 0 in fp32.
The levels are small and kappa large (their product decides the gaps).  In a saturated softmax the gradients of the
block's own W1 / W2 are (weighted variance of the level) ~ 0, and what an fp32 run leaves there is rounding noise of size
kappa * level^2 * eps: with levels six times as large the fp32 oracle's own error on the gradient of fwa2_W1 was 3e-3
of its largest entry.  (dense_K = 0 also means that no gradient reaches the long block: family B checks it through
att0 and the gradient of dense_K, family A through everything.)
"""
import numpy as np

from tests.helpers import make_config, p32, random_batch, random_params

# ----------------------------------------------------------------------------- the shapes (d, H, Ls, Sn) and their batches
SHAPES = [(64, 8, 10, 3), (128, 8, 10, 4), (128, 8, 33, 3), (256, 8, 90, 3), (64, 4, 90, 3), (128, 16, 10, 3),
          (128, 4, 33, 2), (256, 8, 10, 2), (128, 8, 10, 40), (64, 8, 10, 37)]
# family B: the register window at d = 64 / 128 / 256, both streamed widths (one and two 16-channel blocks per column),
# a long-session case at d = 64 and at d = 128
SHAPES_B = [(64, 8, 10, 3), (128, 8, 10, 4), (256, 8, 10, 2), (128, 8, 33, 3), (64, 4, 90, 3), (256, 8, 90, 3),
            (128, 8, 10, 40), (64, 8, 10, 37)]


def batch_size(d, H, Ls, Sn):
    """19-24 samples; 40 at d = 64, Ls = 10, Sn = 3: more than one pass of 16 samples, the last one not full."""
    if (d, H, Ls, Sn) == (64, 8, 10, 3):
        return 40
    if Ls > 33:
        return 24          # (room for every chunk boundary of a 90-entry window in the planted profiles)
    return 19 + (d // 64 + H + Ls + Sn) % 6


def case_id(shape):
    return "d%d-H%d-Ls%d-Sn%d" % shape


def config_for(shape, B, **kw):
    d, H, Ls, _ = shape
    return make_config(U=max(50, B + 7), I=150, C=8, d=d, H=H, Ls=Ls, regulation_rate=1e-3, **kw)


# ----------------------------------------------------------------------------- family A
SHARPNESS = 30.0
# 8 channels per head give the smallest score spread and the flattest attention of the shapes: they need more for half
# of their softmaxes to pass 0.9, and a long session more again (tests/test_saturated_cpu.py asserts that of every case)
SHARPNESS_OF = {(64, 8, 10, 3): 60.0, (128, 16, 10, 3): 60.0, (64, 8, 10, 37): 90.0}


def sharpened(shape, seed=None, S=None, test=False):
    """-> cfg, params (fp32-rounded, as float64), batch, item -> category map."""
    d, H, Ls, Sn = shape
    B = batch_size(*shape)
    seed = d + H + Ls + Sn if seed is None else seed
    S = SHARPNESS_OF.get(shape, SHARPNESS) if S is None else S
    cfg = config_for(shape, B)
    p = random_params(cfg, seed=seed)
    for k in ("fwa1_W2", "fwa2_W2"):
        p[k] = p[k] * S
    p = p32(p)
    b, cat = random_batch(cfg, B=B, Sn=Sn, seed=seed + 1, test=test)
    b["sl"][:3] = [Ls, 1, Ls - 1]          # a full window, a single entry, a masked tail of one
    ar = np.arange(Ls)[None, :]
    b["hist_i"] = np.where(ar < b["sl"][:, None], np.random.RandomState(seed + 2).randint(0, cfg["item_count"], (B, Ls)), 0)
    b["hist_t"] = np.where(ar < b["sl"][:, None], 1.0 / np.random.RandomState(seed + 3).randint(1, 13, (B, Ls)), 0).astype(np.float32)
    assert (b["sl"] < Ls).any() and (b["sl_new"] < Sn).any()
    return cfg, p, b, cat


# ----------------------------------------------------------------------------- family B
C1, KAPPA, BETA = 0.75, 160.0, 0.9375    # W1 = C1 I, W2 = KAPPA I, b1 = BETA > C1 * 0.8 * (largest |level| = MID + A_C)
KC = C1 * KAPPA                       # alpha = KC * sigma: nats per unit of level
A_M, A_C, RAMP, MID, RISE = 0.21, 1.3, 0.025, 0.125, 0.02
GAMMA, HT = 1.25, 0.5                 # s_t = GAMMA * usert_emb[u, t] * HT


def chunk_lengths(d, H):
    """(entries of a chunk of the streamed long block, ids of a session prefetch chunk) as tlsan_attn.h has them:
    NLc = 4 * CPS with CPS = d / max(16, d / H) columns per sample (Geo, tlsan_common.h) -- 16 or 32; a session chunk is
    NL = NLK = 16 keys where the window is in registers and a column is one 16-channel block (LKEY, tlsan_attn_lds.h),
    4 * CPS ids otherwise.  Whichever applies, the chunks end at multiples of 16: the boundary profiles put a peak on
    both sides of EVERY multiple of 16 they have room for, so each real boundary is among them."""
    cps = d // max(16, d // H)
    return 4 * cps, (16 if d // H <= 16 else 4 * cps)


def _ramp(n, rng):
    """n distinct levels in (0, RAMP], none of them 0"""
    return (rng.permutation(n) + 1.0) * (RAMP / max(n, 1))


def profile_levels(name, n, rng, at=None):
    """The levels of n positions (first position 0) for profile `name` -> (levels, peak, anti): the positions of the
    largest and of the smallest level where the profile plants one (None where it does not).
      rise / fall        strictly monotone: a channel replaces its running maximum at every position, or never
      peak               a peak at at[0], an anti-peak at at[1]
      tie_all            one level
      tie_two            the same top level at at[0] and at[1], the rest far below
      cliff              at[0] stands A_C above all other positions, which tie"""
    lv = _ramp(n, rng)
    peak = anti = None
    if name in ("rise", "fall"):
        lv = np.arange(n) * min(RISE, 40 * RISE / max(n, 1)) * (1.0 if name == "rise" else -1.0)
        peak, anti = (n - 1, 0) if name == "rise" else (0, n - 1)
    elif name == "peak":
        peak = min(at[0], n - 1)
        lv[peak] = A_M + RAMP
        if n > 1 and min(at[1], n - 1) != peak:
            anti = min(at[1], n - 1)
            lv[anti] = -A_M
    elif name == "tie_all":
        lv = np.zeros(n)
    elif name == "tie_two":
        lv = -A_M - lv
        lv[min(at[0], n - 1)] = lv[min(at[1], n - 1)] = 0.0
    elif name == "cliff":
        lv = np.zeros(n)
        peak = min(at[0], n - 1)
        lv[peak] = A_C
    else:
        raise ValueError(name)
    return lv, peak, anti


def _plans(n_max, boundaries, B, rng, short):
    """One (profile, length, at) per sample: every profile, the peak placements in both orientations, the chunk
    boundaries that fit; lengths below the maximum for most samples, the maximum for some."""
    last = n_max - 1
    plans = [("peak", None, (0, 10 ** 6)), ("peak", None, (10 ** 6, 0)), ("cliff", None, (10 ** 6,)), ("rise", None, None),
             ("fall", None, None), ("tie_all", None, None), ("tie_two", None, (0, 10 ** 6)), ("cliff", None, (0,)),
             ("peak", n_max, (last, 0)), ("peak", n_max, (0, last))]
    plans += [("cliff", None, (1,)), ("tie_two", None, (1, 2)), ("peak", 1, (0, 0)), ("peak", None, (1, 0))]
    for k in boundaries:                       # the last position of a chunk and the first of the next, both ways
        if k < n_max:
            plans += [("peak", None, (k - 1, k)), ("peak", None, (k, k - 1))]
    out = []
    for s in range(B):
        name, n, at = plans[s % len(plans)]
        if n is None:
            lo = 3 if name != "peak" else (1 if short else 2)   # (ties, cliffs and monotone runs need positions to show on)
            if at is not None:
                lo = max(lo, 1 + max((x for x in at if x < 10 ** 6), default=0))
            lo = min(lo, n_max)
            # (most samples keep a masked tail; those that need position k + 1 to exist may end up full)
            n = int(rng.randint(lo, max(lo, n_max - 1) + 1))
        out.append((name, n, at))
    return out


def planted(shape, seed=0, test=False):
    """-> cfg, params (fp32-rounded, as float64), batch, item -> category map, info.  info: per block ('long' /
    'short') the profile, the length and the positions of the planted peak and anti-peak of every sample, and `sigma`."""
    d, H, Ls, Sn = shape
    B = batch_size(*shape)
    rng = np.random.RandomState(1000 + seed + d + H + Ls + Sn)
    dh, di = d // H, d // 2
    sigma = rng.uniform(0.6, 0.8, d) * rng.permutation(np.where(np.arange(d) % 2 == 0, 1.0, -1.0))
    mult16 = [k for k in range(16, 96, 16)]
    plans_l = _plans(Ls, mult16, B, rng, short=False)
    plans_s = _plans(Sn + 1, [k + 1 for k in mult16], B, rng, short=True)   # (session entry k is position k + 1)
    # the two blocks' profiles are dealt out with different offsets, so that a sample pairs two different ones
    plans_s = plans_s[5:] + plans_s[:5]
    # ---- long block: levels through usert_emb
    U = B + 9
    users = rng.permutation(U)[:B]
    usert = rng.uniform(-1.0, 1.0, (U, Ls))              # (masked tails and unused users: must not matter)
    hist_t = np.zeros((B, Ls), np.float32)
    hist_i = np.zeros((B, Ls), np.int64)
    sl = np.zeros(B, np.int64)
    info = dict(sigma=sigma, long=[], short=[])
    for s, (name, n, at) in enumerate(plans_l):
        lv, peak, anti = profile_levels(name, n, rng, at)
        sl[s] = n
        hist_t[s, :n] = HT
        hist_i[s, :n] = 1 + s % 2                        # item 1 (level +1) or item 2 (level -1) at every valid position
        usert[users[s], :n] = lv / (GAMMA * HT)
        zero = None
        if name == "peak" and n >= 4 and s % 3 == 0:     # a valid position with hist_t = 0: input 0, level 0
            zero = [t for t in range(n) if t not in (peak, anti)][n // 2 - 1]
            hist_t[s, zero] = 0.0
        if s % 2:                                        # item 2 flips every level
            peak, anti = anti, peak
        info["long"].append(dict(profile=name, n=n, peak=peak, anti=anti, zero=zero))
    # ---- short block: levels through planted item / category rows
    level_id = {}
    levels = [0.0, 1.0, -1.0]                            # id 0 (padding), 1 and 2 (the windows' items)

    def item_of(level):
        key = round(float(level), 9)
        if key not in level_id:
            level_id[key] = len(levels)
            levels.append(key)
        return level_id[key]

    hist_i_new = np.zeros((B, Sn), np.int64)
    sl_new = np.zeros(B, np.int64)
    for s, (name, n, at) in enumerate(plans_s):
        lv, peak, anti = profile_levels(name, n, rng, at)
        lv = lv + (MID - lv[0])                          # position 0 is the bridge, whose level is MID
        sl_new[s] = n - 1
        hist_i_new[s, :n - 1] = [item_of(x) for x in lv[1:]]
        info["short"].append(dict(profile=name, n=n, peak=peak, anti=anti, zero=None))
    assert (sl < Ls).any() and (sl_new < Sn).any() and (sl == Ls).any() and (sl_new == Sn).any()
    # the candidates i / j are items of their own with small random rows (and categories of their own): a candidate at a
    # cliff's level, with u_t at one too, would make logits of hundreds, which fp32 cannot hold to 1e-4
    NC = 16
    n_lv = len(levels)
    I = C = n_lv + NC
    lvl = np.asarray(levels + [0.0] * NC)
    assert np.abs(lvl).max() <= MID + A_C and BETA > C1 * 0.8 * (MID + A_C)
    cfg = make_config(U=U, I=I, C=C, d=d, H=H, Ls=Ls, regulation_rate=1e-3)
    p = random_params(cfg, seed=seed + 5)
    p["gamma"] = np.array(GAMMA)
    p["usert_emb"] = usert
    p["item_emb"] = lvl[:, None] * sigma[None, :di]
    p["cate_emb"] = lvl[:, None] * sigma[None, di:]
    p["item_emb"][n_lv:] = rng.uniform(-0.25, 0.25, (NC, di))
    p["cate_emb"][n_lv:] = rng.uniform(-0.25, 0.25, (NC, d - di))
    p["dense_K"] = np.zeros((d, d))
    p["dense_b"] = MID * sigma
    for blk in ("fwa1", "fwa2"):
        p[blk + "_W1"] = C1 * np.eye(dh)
        p[blk + "_b1"] = np.full(dh, BETA)
        p[blk + "_W2"] = KAPPA * np.eye(dh)              # (b2 stays random: it must cancel)
    p = p32(p)
    cat = np.arange(I, dtype=np.int32)                   # item k's category row carries item k's level
    b = dict(u=users.astype(np.int64), i=rng.randint(n_lv, I, B).astype(np.int64), hist_i=hist_i, hist_i_new=hist_i_new,
             hist_t=hist_t, sl=sl, sl_new=sl_new, u_cate=rng.randint(n_lv, C, B).astype(np.int64))
    if test:
        b["j"] = rng.randint(n_lv, I, B).astype(np.int64)
    else:
        b["y"] = rng.randint(0, 2, B).astype(np.float32)
    return cfg, p, b, cat, info


def planted_scores(p, cat, b, H):
    """The closed form: the planted linear scores kappa (c x + beta) + b2 of both blocks, from the parameters and the
    batch alone (no matrix product, no relu) -> (scores [B, Ls, d], scores [B, 1 + Sn, d], smallest c x + beta)."""
    d = p["dense_b"].shape[0]
    row = lambda ids: np.concatenate([p["item_emb"][ids], p["cate_emb"][np.asarray(cat, np.int64)[ids]]], -1)
    s = p["gamma"] * p["usert_emb"][b["u"]] * b["hist_t"].astype(np.float64)
    x0 = row(b["hist_i"]) * s[:, :, None]
    x1 = np.concatenate([np.broadcast_to(p["dense_b"], (len(b["u"]), 1, d)), row(b["hist_i_new"])], 1)
    out, zmin = [], np.inf
    for x, blk in ((x0, "fwa1"), (x1, "fwa2")):
        c, beta = p[blk + "_W1"][0, 0], np.tile(p[blk + "_b1"], H)
        kappa, b2 = p[blk + "_W2"][0, 0], np.tile(p[blk + "_b2"], H)
        z = c * x + beta
        zmin = min(zmin, z.min())
        out.append(kappa * z + b2)
    return out[0], out[1], zmin


def masked_softmax(scores, length):
    """softmax over axis 1 of the first length[b] positions; 0 past them"""
    valid = np.arange(scores.shape[1])[None, :, None] < np.asarray(length)[:, None, None]
    sc = np.where(valid, scores, -np.inf)
    e = np.exp(sc - sc.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ----------------------------------------------------------------------------- large logits
LOGIT_TARGETS = (20.0, -20.0, 60.0, -60.0, 100.0, -100.0)


def plant_logits(p, cat, b, H):
    """item_b such that the first 12 samples' logits are +-20, +-60, +-100, each under label 0 and label 1 (their
    candidates made distinct items).  -> params, batch, the targets [12]"""
    from oracle import tlsan_oracle as orc
    p, b = {k: v.copy() for k, v in p.items()}, {k: v.copy() for k, v in b.items()}
    n = 2 * len(LOGIT_TARGETS)
    I = p["item_b"].shape[0]
    assert len(b["i"]) >= n and I >= len(b["i"])
    b["i"] = (np.arange(len(b["i"])) * 7 + 3) % I if np.gcd(7, I) == 1 else np.arange(len(b["i"])) % I
    assert len(set(b["i"].tolist())) == len(b["i"])
    want = np.repeat(LOGIT_TARGETS, 2)
    b["y"][:n] = np.tile([0.0, 1.0], len(LOGIT_TARGETS))
    base = orc.forward(p, cat, b, H)["logits"][:n] - p["item_b"][b["i"][:n]]
    p["item_b"][b["i"][:n]] = want - base
    return p32(p), b, want


# ----------------------------------------------------------------------------- the oracle in both precisions
def to32(p):
    return {k: np.asarray(v, np.float32) for k, v in p.items()}


def att_rows(a, H):
    """the oracle's [B, T, H, dh] attention weights in the layout of Model.att0 / att1: [H * B, T, dh], row h * B + b"""
    B, T, _, dh = a.shape
    return np.asarray(a).transpose(2, 0, 1, 3).reshape(H * B, T, dh)


def rel_err(a, ref):
    """largest error as a fraction of the largest entry of the reference"""
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / (np.abs(ref).max() + 1e-300))


# ----------------------------------------------------------------------------- a case and its reference, computed once
LR = 0.6
_CASES = {}


def reference(p, cat, b, H, reg, dropout=None):
    """The fp64 oracle on (p, b) -- forward for candidates i and j, gradients, both norms, one SGD step at LR -- and
    `e32`: the error of the same oracle run in fp32 on the same inputs, per compared quantity (absolute; 'n18' / 'nd'
    relative; 'upd' is the error of the update lr * coef * g)."""
    from oracle import tlsan_oracle as orc
    out = []
    for q in (p, to32(p)):
        r = dict(fwd=orc.forward(q, cat, b, H))
        if "j" in b:
            r["fwd_j"] = orc.forward(q, cat, dict(b, i=b["j"]), H)
        with np.errstate(over="ignore"):          # (fp32: exp(100) = inf in the sigmoid of a planted logit, 1 / inf = 0 is right)
            loss, logits, g, sparse = orc.backward(q, cat, b, H, reg, dropout=dropout)
        r.update(loss=float(loss), logits=logits, g=g, n18=orc.global_norm(q, g, sparse, reg, "tf18"),
                 nd=orc.global_norm(q, g, sparse, reg, "dedup"))
        r["coef"] = 5.0 / max(r["n18"], 5.0)
        r["upd"] = {k: -LR * r["coef"] * np.asarray(g[k], np.float64) for k in g}
        out.append(r)
    ref, r32 = out
    ref["newp"] = {k: p[k] + ref["upd"][k] for k in p}
    amax = lambda a, c: float(np.abs(np.asarray(a, np.float64) - c).max())
    e = dict(logits=amax(r32["fwd"]["logits"], ref["fwd"]["logits"]), u_t=amax(r32["fwd"]["u_t"], ref["fwd"]["u_t"]),
             att0=amax(r32["fwd"]["att0"], ref["fwd"]["att0"]), att1=amax(r32["fwd"]["att1"], ref["fwd"]["att1"]),
             loss=abs(r32["loss"] - ref["loss"]), n18=abs(r32["n18"] - ref["n18"]) / ref["n18"],
             nd=abs(r32["nd"] - ref["nd"]) / ref["nd"],
             g={k: amax(r32["g"][k], ref["g"][k]) for k in ref["g"]},
             upd={k: amax(r32["upd"][k], ref["upd"][k]) for k in ref["g"]})
    if "j" in b:
        e["logits_j"] = amax(r32["fwd_j"]["logits"], ref["fwd_j"]["logits"])
    ref["e32"] = e
    return ref


def case(family, shape):
    """family 'A' (sharpened) or 'B' (planted) at `shape`: inputs (with labels y AND a second candidate j) and reference,
    built once per process and shared by the tests, which leave them unchanged."""
    key = (family, tuple(shape))
    if key not in _CASES:
        if family == "A":
            cfg, p, b, cat = sharpened(shape)
            info = None
        else:
            cfg, p, b, cat, info = planted(shape)
        b["j"] = b["i"][::-1].copy()
        H = shape[1]
        ref = reference(p, cat, b, H, cfg["regulation_rate"])
        _CASES[key] = dict(cfg=cfg, p=p, b=b, cat=cat, info=info, H=H, ref=ref, shape=tuple(shape))
    return _CASES[key]


def tol(existing, e32):
    """The tolerance of a compared quantity: what the suite already uses for it, or 4 x the fp32 oracle's own error on
    the same inputs where that is larger (the kernel differs from an fp32 oracle by a handful of roundings of that size:
    MFMA accumulation order, the log2(e) pre-scale of W2, v_exp_f32, the fast reciprocal)."""
    return max(existing, 4.0 * e32)

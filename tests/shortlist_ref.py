"""Numpy reference of the bf16 shortlist index (tlsan_shortlist_build / _topk / _select, recommend's index=<ShortlistIndex>):
the bf16 rounding (nearest even) of both operands, the approximate scores in float64 from the rounded operands, the
shortlist in tf.nn.top_k's order (tests/scope_ref.py's selection), the bound eps_b and the certificate.  The exact scores are
not restated here: the tests pass the exact path's own (score_candidates' / recommend's), whose bits the feature promises."""
import numpy as np

from tests import scope_ref

C = 2.0 ** -7 + 2.0 ** -11      # the certificate's constant (DESIGN.md section 7 derives it)


def bf16_bits(x):
    """float32 -> the uint16 pattern of its bfloat16, round to nearest even (NaN stays a NaN)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(b):
    """uint16 bfloat16 patterns -> float32"""
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def wmax(w):
    """max_n ||w_n||_2 of the stored fp32 rows, in float64"""
    return float(np.sqrt((np.asarray(w, np.float32).astype(np.float64) ** 2).sum(1)).max())


def approx_scores(ut, w, P, bias):
    """a~ [B, I] in float64 from the rounded operands, and sum_k |u~_k w~_k| [B, I] (what the kernel's fp32 error scales with)"""
    u = bf16_round(ut).astype(np.float64)
    v = bf16_round(w).astype(np.float64)
    return (u @ v.T) * float(P) + np.asarray(bias, np.float64)[None, :], np.abs(u) @ np.abs(v).T


def stage1_tolerance(d, P, absprod, approx):
    """|a~_gpu - a~_ref| <= d 2^-23 |P| sum|u~ w~| + 2^-22 |a~_ref|: the products of two bf16 values are exact in fp32, then d
    fp32 accumulations (each within 2^-24 of a partial sum that sum|u~ w~| bounds, with room for the order) and the two
    roundings of the scale and the bias."""
    return d * 2.0 ** -23 * abs(float(P)) * absprod + 2.0 ** -22 * np.abs(approx)


def shortlist(approx, ok, N):
    """ids [B, N] (global ids are the column numbers; -1 padding) and their approximate scores"""
    return scope_ref.topk(approx, ok, N)


def epsilon(ut, P, wm, sK, aN):
    """eps_b of the rows: c |P| ||u_t[b]||_2 wmax + 2^-20 (|s_K| + |a~_N|)"""
    norm = np.sqrt((np.asarray(ut, np.float32).astype(np.float64) ** 2).sum(1))
    with np.errstate(invalid="ignore", over="ignore"):
        return C * abs(float(P)) * norm * float(wm) + 2.0 ** -20 * (np.abs(sK) + np.abs(aN))


def certify(exact, approx, ok, N, K, ut, P, wm, eps_scale=1.0):
    """The whole second stage from the exact path's [B, I] scores: -> (ids [B, K], scores [B, K], certified [B] bool, eps [B],
    gap [B] = s_K - a~_N, NaN where the shortlist is short).  eps_scale: a mutant's knob (0: a certificate without its eps)."""
    exact, approx = np.asarray(exact), np.asarray(approx, np.float64)
    B, I = exact.shape
    sid, sap = shortlist(approx, ok, N)
    ids = np.full((B, K), -1, np.int32)
    sc = np.full((B, K), -np.inf, exact.dtype)
    cert = np.zeros(B, bool)
    sK, aN = np.full(B, np.nan), np.full(B, np.nan)
    for b in range(B):
        inside = np.zeros(I, bool)
        inside[sid[b][sid[b] >= 0]] = True
        i1, s1 = scope_ref.topk(exact[b:b + 1], inside[None, :], K)
        ids[b], sc[b] = i1[0], s1[0]
        if sid[b, N - 1] < 0:
            cert[b] = True
        else:
            sK[b], aN[b] = float(s1[0, K - 1]), sap[b, N - 1]
    eps = epsilon(ut, P, wm, sK, aN)
    with np.errstate(invalid="ignore"):
        full = ~cert
        cert |= full & np.isfinite(sK) & np.isfinite(aN) & np.isfinite(eps) & (sK > aN + eps_scale * eps)
    return ids, sc, cert, eps, sK - aN


# ---- the rounding counter-example: what a certificate without its eps term gets wrong, with a shortlist of N entries ----
def counter_example(d, N):
    """u_t [1, d] and I = N + 1 items (A, N - 1 copies of B, O) with zero biases: O's bf16 score ties B's, so with the
    tie going to the lower id O is the one item outside the shortlist -- and O's exact score beats A's, the best inside."""
    ut = np.zeros((1, d), np.float32)
    ut[0, 0], ut[0, 1] = 1.0, 1.0 + 2.0 ** -8 - 2.0 ** -20
    w = np.zeros((N + 1, d), np.float32)
    w[0, 0] = 1.0 + 2.0 ** -6 + 2.0 ** -7                  # A
    w[1:N, 0] = 1.0 + 2.0 ** -6                            # B
    w[N, 1] = 1.0 + 2.0 ** -6 + 2.0 ** -8 - 2.0 ** -20     # O
    return ut, w

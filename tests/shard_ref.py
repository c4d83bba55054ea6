"""The references of the sharded step's owner-side calls (include/tlsan.h: tlsan_shard_apply / _opt, tlsan_shard_apply_lazy,
tlsan_shard_summary / _opt, tlsan_shard_gather_wire_bf16) in numpy fp64.  No torch, no GPU.  Scalars that a kernel receives
as fp32 (gscale, reg, lr, step_dev[*], P) are rounded to fp32 by the CALLER and widened here: nothing in this file rounds,
so that the identities between the forms (tests/test_shard_ref_cpu.py) hold to fp64 rounding."""
import numpy as np

U32 = 2.0 ** -24      # unit roundoff of fp32: the unit of the element bounds of tests/test_gpu_shard_kernels.py


def _np_opt_elem(kind, lr, b1, b2, eps, step, w, g, s1, s2):
    """opt_elem of csrc/tlsan_opt.h in float64 (TF 1.8's Adam / RMSProp / Adadelta)"""
    if kind == "adam":
        s1 = s1 * b1 + g * (1.0 - b1)
        s2 = s2 * b2 + g * g * (1.0 - b2)
        alpha = lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
        return w - alpha * s1 / (np.sqrt(s2) + eps), s1, s2
    if kind == "rmsprop":
        s1 = s1 * b1 + g * g * (1.0 - b1)
        s2 = s2 * b2 + lr * g / np.sqrt(s1 + eps)
        return w - s2, s1, s2
    s1 = s1 * b1 + g * g * (1.0 - b1)
    upd = np.sqrt(s2 + eps) / np.sqrt(s1 + eps) * g
    return w - upd * lr, s1, s2 * b1 + upd * upd * (1.0 - b1)


def reg_cols(R, cI, reg_item, reg_user):
    """[R] number of regularised columns of every shard row: items [0, cI), users [cI, R)"""
    return np.where(np.arange(R) < cI, reg_item, reg_user)


def source_sum(R, W, rows, src_off, vals):
    """-> (sum [R, W] of the received rows over the sources in fp64, received [R] bool).  rows [n_recv] concatenated in source
    order, src_off [G + 1]; the rows of one source are distinct."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    src_off = np.asarray(src_off, np.int64)
    assert src_off[0] == 0 and src_off[-1] == len(rows) and (np.diff(src_off) >= 0).all()
    for s in range(len(src_off) - 1):
        part = rows[src_off[s]:src_off[s + 1]]
        assert len(np.unique(part)) == len(part), "the rows of one source are distinct"
    acc = np.zeros((R, W))
    got = np.zeros(R, bool)
    if len(rows):
        np.add.at(acc, rows, np.asarray(vals, np.float64)[:, :W])
        got[rows] = True
    return acc, got


def apply_dense(shard0, cate0, rows, src_off, vals, g_cate, cI, W, reg_item, reg_user, gscale, step, coef, reg, opt=None):
    """tlsan_shard_apply (opt None) / tlsan_shard_apply_opt: every row r < R, every column c < W
        g = gscale * sum over the sources + (reg * w on the first reg_cols(r) columns)
    SGD: w -= step * g.  Otherwise _np_opt_elem on coef * g for every column c < W, except item_b (column reg_item of an item
    row), which keeps its weight and both accumulators where g == 0 unless the kind is Adam.  Category rows:
    g = gscale * g_cate + reg * w on all dc columns.  shard0 [R, >= W] (columns past W are carried along unchanged).
    opt: dict(kind, lr, b1, b2, eps, step, shard_s1, shard_s2, cate_s1, cate_s2), the accumulators laid out like the tables.
    -> (shard, cate, accumulators (dict of the four, or None), (sum of squares of the shard's regularised columns, of cate))"""
    w = np.array(shard0, np.float64)
    c = np.array(cate0, np.float64)
    R = w.shape[0]
    gscale, step, coef, reg = (np.float64(x) for x in (gscale, step, coef, reg))
    acc, _ = source_sum(R, W, rows, src_off, vals)
    nreg = reg_cols(R, cI, reg_item, reg_user)
    rg = np.arange(W)[None, :] < nreg[:, None]
    g = gscale * acc + np.where(rg, reg * w[:, :W], 0.0)
    gc = gscale * np.asarray(g_cate, np.float64) + reg * c
    slots = None
    if opt is None or opt["kind"] == "sgd":
        w[:, :W] -= step * g
        c -= step * gc
    else:
        slots = {k: np.array(opt[k], np.float64) for k in ("shard_s1", "shard_s2", "cate_s1", "cate_s2")}
        o = (opt["kind"], np.float64(opt["lr"]), opt["b1"], opt["b2"], opt["eps"], opt["step"])
        move = np.ones((R, W), bool)
        if opt["kind"] != "adam" and reg_item < W:
            move[:cI, reg_item] = g[:cI, reg_item] != 0.0
        nw, n1, n2 = _np_opt_elem(*o, w[:, :W], coef * g, slots["shard_s1"][:, :W], slots["shard_s2"][:, :W])
        w[:, :W] = np.where(move, nw, w[:, :W])
        slots["shard_s1"][:, :W] = np.where(move, n1, slots["shard_s1"][:, :W])
        slots["shard_s2"][:, :W] = np.where(move, n2, slots["shard_s2"][:, :W])
        c, slots["cate_s1"], slots["cate_s2"] = _np_opt_elem(*o, c, coef * gc, slots["cate_s1"], slots["cate_s2"])
    return w, c, slots, (float((w[:, :W] ** 2)[rg].sum()), float((c ** 2).sum()))


def apply_lazy(shard0, cate0, rows, src_off, vals, g_cate, cI, W, reg_item, reg_user, gscale, step_dev4):
    """tlsan_shard_apply_lazy on the STORED tables (true table = P * stored on the regularised columns): only received rows
    move, stored w -= step_dev[2] * gscale * sum on the columns below reg_cols(r), w -= step_dev[0] * gscale * sum on
    [reg_cols, W); every category row w -= step_dev[2] * gscale * g_cate.
    -> (shard, cate, P_new = step_dev[3], change of the shard's regularised sum of squares, cate's sum of squares)"""
    w = np.array(shard0, np.float64)
    c = np.array(cate0, np.float64)
    R = w.shape[0]
    sd = [np.float64(x) for x in step_dev4]
    gscale = np.float64(gscale)
    acc, got = source_sum(R, W, rows, src_off, vals)
    rg = np.arange(W)[None, :] < reg_cols(R, cI, reg_item, reg_user)[:, None]
    before = (w[:, :W] ** 2)[rg].sum()
    new = w[:, :W] - np.where(rg, sd[2], sd[0]) * (gscale * acc)
    w[:, :W] = np.where(got[:, None], new, w[:, :W])
    c -= sd[2] * (gscale * np.asarray(g_cate, np.float64))
    return w, c, sd[3], float((w[:, :W] ** 2)[rg].sum() - before), float((c ** 2).sum())


def summary(flat, n_dense, n_cate, G, lr, reg, clip, S_cate, P=None, opt=None, dense=None):
    """tlsan_shard_summary / _opt after the all-reduce of flat = [dense grads | cate grads | BCE, row squares, table squares | pad].
    opt: dict(kind, b1, b2, eps, step, dense_s1, dense_s2) for the dense weights (None: SGD); dense: the weights (optional).
    -> dict(norm, coef, step, S_tot, loss, loss_scale, step_dev [2 without P, 4 with], dense, dense_s1, dense_s2)"""
    flat = np.asarray(flat, np.float64)
    lr, reg, clip, S_cate = (np.float64(x) for x in (lr, reg, clip, S_cate))
    tail = flat[n_dense + n_cate:]
    Pv = np.float64(1.0 if P is None else P)
    S_tot = (tail[2] + S_cate) * Pv * Pv
    gd = flat[:n_dense] / G
    norm = np.sqrt(tail[1] / (G * G) + reg * reg * S_tot + (gd * gd).sum())
    coef = np.float64(1.0) if norm <= clip else clip / norm
    step = lr * coef
    out = dict(norm=norm, coef=coef, step=step, S_tot=S_tot, loss=tail[0] / G + reg / 2 * S_tot,
               loss_scale=abs(tail[0] / G) + abs(reg / 2 * S_tot), step_dev=[step, coef], dense=None, dense_s1=None, dense_s2=None)
    if P is not None:
        P_new = Pv * (1.0 - step * reg)
        out["step_dev"] = [step, coef, step / P_new, P_new]
    if dense is not None:
        w = np.array(dense, np.float64)
        if opt is None or opt["kind"] == "sgd":
            out["dense"] = w - step * gd
        else:
            out["dense"], out["dense_s1"], out["dense_s2"] = _np_opt_elem(
                opt["kind"], lr, opt["b1"], opt["b2"], opt["eps"], opt["step"], w, coef * gd,
                np.array(opt["dense_s1"], np.float64), np.array(opt["dense_s2"], np.float64))
    return out


def bf16_rne_bits(x_f32):
    """fp32 -> bf16, round to nearest even, on the bit patterns (no NaN handling) -> uint16"""
    b = np.ascontiguousarray(x_f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


# fp32 bit patterns whose rounding to bf16 is worth planting: ties with an even and an odd kept bit, their neighbours,
# signed zeros and infinities, and the largest finite fp32 (which becomes inf) -> the bf16 bits each must give
BF16_PLANTED = [(0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81),
                (0x00000000, 0x0000), (0x80000000, 0x8000), (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
                (0x7F7FFFFF, 0x7F80), (0xFF7FFFFF, 0xFF80)]

"""The owner-side calls of the row-sharded step, one by one, against tests/shard_ref.py (numpy, fp64): tlsan_shard_apply,
tlsan_shard_apply_opt, tlsan_shard_apply_lazy, tlsan_shard_apply_lazy_static, tlsan_shard_summary / _opt, tlsan_shard_gather,
tlsan_shard_gather_wire_bf16 and tlsan_scan_compact through ctypes, in one process.  One GPU plays an owner that receives
from up to 16 sources: the received buffers are made up here (as test_apply_lazy_opt_against_numpy does), with three row
strides that all differ, source counts on both sides of the kernels' four-at-a-time loop, and rows on both sides of the
item / user boundary.

Element bounds, u = 2^-24 (derived, not tuned; tests/test_shard_ref_cpu.py reaches 2.8 u S with the arithmetic they allow):
  SGD forms      |got - ref| <= 8 u S,  S = |w0| + step (gscale |sum| + reg |w0|)  (dense),  |w0| + s gscale |sum|  (lazy)
  optimizers     the bounds of test_apply_lazy_opt_against_numpy: 1e-5 of the largest move + 1e-7, slots 1e-5 relative
  sums of squares  1e-9 relative to max(1, |value|) against the fp64 sum over the device's own output
  summary scalars  16 u relative
Every case runs twice on fresh copies of its input and must leave the same bits.  Each test prints the worst error it saw
in the units of its bound (`record ...` lines, shown with -s): profiles/shard_kernel_tests.md keeps one run's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import shard_ref as sr
from tests.helpers import make_config

pytestmark = pytest.mark.gpu

U = sr.U32
R, CI, CN = 330, 150, 37                 # none a multiple of the 16 rows a workgroup takes
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
F32 = np.float32
# (reg_item, reg_user, W, dc); the last is the widest row the dense form takes
WIDTHS = [(32, 42, 44, 32), (64, 74, 76, 64), (128, 218, 220, 128), (128, 256, 256, 256)]
# (G, index into WIDTHS, source left empty or None): every G at W = 76 (one trip of the dense kernel's four-source loop, a
# partial trip, an exact one, two with a partial second, four), every width at G = 5
GEOMETRY = [(1, 1, None), (3, 1, 0), (4, 1, None), (5, 1, None), (16, 1, None), (5, 0, None), (5, 2, 4), (5, 3, None)]
GEOMETRY_IDS = ["G%d-W%d%s" % (g, WIDTHS[w][2], "" if e is None else "-src%d-empty" % e) for g, w, e in GEOMETRY]


def _lib():
    from tlsan_amd import _lib as L
    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def record(name, **kw):
    print("record %s %s" % (name, " ".join("%s=%.3g" % kv for kv in sorted(kw.items()))))


def step_dev_for(G, P=None, lr=0.05, reg=1e-2):
    """step_dev as tlsan_shard_summary_opt would leave it for a clip that bites (coef ~ 0.37), from the reference, rounded to
    the fp32 the apply kernels read -> (fp32 [4], lr, reg as fp32)"""
    rng = np.random.RandomState(100 + G)
    flat = np.concatenate([rng.randn(6), [0.7, 3.0 * G * G, 50.0, 0.0]]).astype(F32)
    free = sr.summary(flat, 4, 2, G, F32(lr), F32(reg), F32(1e30), 3.0, P=P)
    s = sr.summary(flat, 4, 2, G, F32(lr), F32(reg), F32(0.37 * free["norm"]), 3.0, P=P)
    assert abs(s["coef"] - 0.37) < 1e-3
    sd = np.zeros(4, F32)
    sd[:len(s["step_dev"])] = s["step_dev"]
    return sd, F32(lr), F32(reg)


_CASES = {}


def received(G, wi, empty, seed_extra=0):
    """The made-up input of one owner update: per source a sorted, distinct choice of 20-60 rows, plus rows 0, cI-1, cI and
    R-1 from some source, one item row and one user row from every source, one row from source G-1 alone; `empty` names a
    source that sends nothing (src_off[s] == src_off[s+1]).  Built once per geometry and never written to."""
    key = (G, wi, empty, seed_extra)
    if key in _CASES:
        return _CASES[key]
    ri, ru, W, dc = WIDTHS[wi]
    ld, ldv = W + 4, W + 8
    rng = np.random.RandomState(1000 * G + 10 * wi + seed_extra)
    ALL_I, ALL_U, LAST = 7, CI + 9, 11
    per = [set(rng.choice(R, rng.randint(20, 61), replace=False).tolist()) - {LAST} for _ in range(G)]
    sending = [s for s in range(G) if s != empty]
    for r in (0, CI - 1, CI, R - 1):
        per[sending[rng.randint(len(sending))]].add(r)
    for s in range(G):
        per[s] |= {ALL_I, ALL_U}
    per[G - 1].add(LAST)
    if empty is not None:
        per[empty] = set()
    per = [np.array(sorted(x), np.int32) for x in per]
    rows = np.concatenate(per).astype(np.int32)
    src_off = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int32)
    n = len(rows)
    vals = np.full((n, ldv), np.nan, F32)                            # (columns [W, ldv): never looked at)
    vals[:, :W] = rng.randn(n, W).astype(F32)
    live = np.where(rows < CI, ri + 1, ru)
    vals[:, :W][np.arange(W)[None, :] >= live[:, None]] = 0.0
    quiet = np.unique(rows[rows < CI])[::3]                          # item rows whose item_b gradient is exactly 0.0
    vals[np.isin(rows, quiet), ri] = 0.0
    shard0 = rng.uniform(-0.8, 0.8, (R, ld)).astype(F32)
    cate0 = rng.uniform(-0.8, 0.8, (CN, dc)).astype(F32)
    g_cate = rng.randn(CN, dc).astype(F32)
    got = np.zeros(R, bool)
    got[rows] = True
    nonempty = [s for s in range(G) if len(per[s])]
    assert got[[0, CI - 1, CI, R - 1]].all() and not got.all()
    assert all(ALL_I in per[s] and ALL_U in per[s] for s in nonempty)
    if empty != G - 1:
        assert LAST in per[G - 1] and not any(LAST in per[s] for s in range(G - 1))
    rg = np.arange(W)[None, :] < sr.reg_cols(R, CI, ri, ru)[:, None]
    lv = np.arange(W)[None, :] < np.where(np.arange(R) < CI, ri + 1, ru)[:, None]
    c = dict(G=G, ri=ri, ru=ru, W=W, dc=dc, ld=ld, ldv=ldv, per=per, rows=rows, src_off=src_off, n=n, vals=vals, quiet=quiet,
             shard0=shard0, cate0=cate0, g_cate=g_cate, got=got, rg=rg, lv=lv, gscale=F32(1.0 / G))
    c["sum"], _ = sr.source_sum(R, W, rows, src_off, vals)
    _CASES[key] = c
    return c


def ref_args(c):
    return (c["rows"], c["src_off"], c["vals"], c["g_cate"], CI, c["W"], c["ri"], c["ru"], c["gscale"])


def check_sums(sq, sq32, want0, want1):
    assert abs(sq[0] - want0) <= 1e-9 * max(1.0, abs(want0)), (sq[0], want0)
    assert abs(sq[1] - want1) <= 1e-9 * max(1.0, abs(want1)), (sq[1], want1)
    assert sq32[0] == np.float32(sq[0])
    return max(abs(sq[0] - want0) / max(1.0, abs(want0)), abs(sq[1] - want1) / max(1.0, abs(want1))) / 1e-9


# ---------------------------------------------------------------------------------------------------------- A, B: dense forms
OPT_LR = {"adam": 0.05, "rmsprop": 0.05, "adadelta": 0.05}     # (as test_apply_lazy_opt_against_numpy)


def run_dense(c, sd, reg, kind, lr, slots0):
    """tlsan_shard_apply (kind sgd) / tlsan_shard_apply_opt on fresh device copies -> dict of host arrays"""
    L, lib = _lib()
    from tlsan_amd.model import OPTIMIZERS
    G, W = c["G"], c["W"]
    shard, cate = dev(c["shard0"]), dev(c["cate0"])
    keep = [dev(x) for x in (c["vals"], c["rows"], c["g_cate"], sd)]
    slots = torch.zeros(R * G, dtype=torch.int32, device="cuda")
    sq = torch.tensor([5.0, 7.0], dtype=torch.float64, device="cuda")
    sq32 = torch.zeros(1, device="cuda")
    nws = int(lib.tlsan_shard_apply_workspace(R, CN))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    so = (C.c_int32 * (G + 1))(*c["src_off"].tolist())
    head = (shard.data_ptr(), c["ld"], CI, R, W, c["ri"], c["ru"], keep[0].data_ptr(), c["ldv"], keep[1].data_ptr(), c["n"], so, G,
            slots.data_ptr(), c["gscale"], keep[3].data_ptr(), reg, cate.data_ptr(), CN, c["dc"], keep[2].data_ptr(),
            sq.data_ptr(), sq32.data_ptr())
    sl = {}
    if kind == "sgd":
        L.check(lib.tlsan_shard_apply(*head, ws.data_ptr(), nws, _stream()), "tlsan_shard_apply")
    else:
        code, b1, b2, eps = OPTIMIZERS[kind]
        sl = {k: dev(v) for k, v in slots0.items()}
        dummy = torch.zeros(4, device="cuda")            # (dense_s1/2: asked for, not looked at by this call)
        opt = L.ShardOptimizer(code, 3, b1, b2, eps, sl["shard_s1"].data_ptr(), sl["shard_s2"].data_ptr(), sl["cate_s1"].data_ptr(),
                               sl["cate_s2"].data_ptr(), dummy.data_ptr(), dummy.data_ptr(), None)
        L.check(lib.tlsan_shard_apply_opt(*head, C.byref(opt), lr, ws.data_ptr(), nws, _stream()), "tlsan_shard_apply_opt")
    out = dict(shard=host(shard), cate=host(cate), slots=host(slots), sq=host(sq), sq32=host(sq32))
    out.update({k: host(v) for k, v in sl.items()})
    return out


def twice(fn):
    a, b = fn(), fn()
    for k in a:
        assert same_bits(a[k], b[k]) if a[k].dtype.kind == "f" else np.array_equal(a[k], b[k]), k
    return a


@pytest.mark.parametrize("G,wi,empty", GEOMETRY, ids=GEOMETRY_IDS)
def test_shard_apply_sgd(G, wi, empty):
    """A. tlsan_shard_apply: every shard row and every category row moves (rows nobody sent by -step reg w), within
    8 u S of the reference; the columns past the live ones and past W keep their bits; slots are zero again on exit."""
    c = received(G, wi, empty)
    sd, _, reg = step_dev_for(G)
    out = twice(lambda: run_dense(c, sd, reg, "sgd", 0.0, None))
    W, d = c["W"], np.float64
    step = d(sd[0])
    ref_w, ref_c, _, _ = sr.apply_dense(c["shard0"], c["cate0"], *ref_args(c), sd[0], sd[1], reg)
    w0 = d(c["shard0"][:, :W])
    S = np.abs(w0) + step * (d(c["gscale"]) * np.abs(c["sum"]) + np.where(c["rg"], d(reg) * np.abs(w0), 0.0))
    err = np.abs(d(out["shard"][:, :W]) - ref_w[:, :W]) / (U * S)
    Sc = np.abs(d(c["cate0"])) + step * (d(c["gscale"]) * np.abs(d(c["g_cate"])) + d(reg) * np.abs(d(c["cate0"])))
    errc = np.abs(d(out["cate"]) - ref_c) / (U * Sc)
    record("apply_sgd[%s]" % GEOMETRY_IDS[GEOMETRY.index((G, wi, empty))], rows_uS=err.max(), cate_uS=errc.max())
    assert err.max() <= 8.0, (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert errc.max() <= 8.0, errc.max()
    moved = bits(out["shard"][:, :W]) != bits(c["shard0"][:, :W])
    assert moved[~c["got"]][c["rg"][~c["got"]]].mean() > 0.9                  # rows nobody sent decay
    assert not moved[~c["lv"]].any()                                          # [live, W): bit for bit
    assert same_bits(out["shard"][:, W:], c["shard0"][:, W:])                 # [W, ld): bit for bit
    assert not out["slots"].any()
    worst = check_sums(out["sq"], out["sq32"], (d(out["shard"][:, :W]) ** 2)[c["rg"]].sum(), (d(out["cate"]) ** 2).sum())
    record("apply_sgd_sums[%s]" % GEOMETRY_IDS[GEOMETRY.index((G, wi, empty))], frac=worst)


def test_shard_apply_nothing_received():
    """n_recv == 0 with vals and rows NULL (G = 3): the decay of every row alone"""
    L, lib = _lib()
    G, (ri, ru, W, dc) = 3, WIDTHS[1]
    ld = W + 4
    rng = np.random.RandomState(5)
    shard0 = rng.uniform(-0.8, 0.8, (R, ld)).astype(F32)
    cate0 = rng.uniform(-0.8, 0.8, (CN, dc)).astype(F32)
    g_cate = rng.randn(CN, dc).astype(F32)
    sd, _, reg = step_dev_for(G)

    def run():
        shard, cate, gc, sdd = dev(shard0), dev(cate0), dev(g_cate), dev(sd)
        slots = torch.zeros(R * G, dtype=torch.int32, device="cuda")
        sq = torch.zeros(2, dtype=torch.float64, device="cuda")
        nws = int(lib.tlsan_shard_apply_workspace(R, CN))
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        L.check(lib.tlsan_shard_apply(shard.data_ptr(), ld, CI, R, W, ri, ru, None, 0, None, 0, (C.c_int32 * (G + 1))(0, 0, 0, 0), G,
                                      slots.data_ptr(), F32(1.0 / G), sdd.data_ptr(), reg, cate.data_ptr(), CN, dc, gc.data_ptr(),
                                      sq.data_ptr(), None, ws.data_ptr(), nws, _stream()), "tlsan_shard_apply")
        return dict(shard=host(shard), cate=host(cate), sq=host(sq), slots=host(slots))

    out = twice(run)
    none = np.zeros(0, np.int32)
    ref_w, ref_c, _, _ = sr.apply_dense(shard0, cate0, none, np.zeros(G + 1, np.int32), np.zeros((0, W), F32), g_cate, CI, W, ri, ru,
                                        F32(1.0 / G), sd[0], sd[1], reg)
    d = np.float64
    rg = np.arange(W)[None, :] < sr.reg_cols(R, CI, ri, ru)[:, None]
    S = np.abs(d(shard0[:, :W])) * (1.0 + d(sd[0]) * d(reg) * rg)
    assert (np.abs(d(out["shard"][:, :W]) - ref_w[:, :W]) <= 8 * U * S).all()
    assert same_bits(out["shard"][:, :W][~rg], shard0[:, :W][~rg]) and same_bits(out["shard"][:, W:], shard0[:, W:])
    assert (bits(out["shard"][:, :W]) != bits(shard0[:, :W]))[rg].mean() > 0.9 and not out["slots"].any()
    Sc = np.abs(d(cate0)) + d(sd[0]) * (d(F32(1.0 / G)) * np.abs(d(g_cate)) + d(reg) * np.abs(d(cate0)))
    assert (np.abs(d(out["cate"]) - ref_c) <= 8 * U * Sc).all()
    assert abs(out["sq"][0] - (d(out["shard"][:, :W]) ** 2)[rg].sum()) <= 1e-9 * out["sq"][0]


@pytest.mark.parametrize("kind", ["adam", "rmsprop", "adadelta"])
@pytest.mark.parametrize("G,wi,empty", GEOMETRY, ids=GEOMETRY_IDS)
def test_shard_apply_opt(G, wi, empty, kind):
    """B. tlsan_shard_apply_opt (Adam at step 3, RMSProp, Adadelta) from accumulators in uniform(1e-3, 2e-3): weights within
    1e-5 of the largest move, accumulators 1e-5 relative; item_b of an item row that was not sent, or whose summed gradient
    is exactly zero, keeps weight and accumulators bit for bit under RMSProp / Adadelta and moves under Adam."""
    from tlsan_amd.model import OPTIMIZERS
    c = received(G, wi, empty)
    sd, _, reg = step_dev_for(G)
    W, ri, d = c["W"], c["ri"], np.float64
    rng = np.random.RandomState(77)
    slots0 = {k: rng.uniform(1e-3, 2e-3, sh).astype(F32) for k, sh in
              (("shard_s1", (R, c["ld"])), ("shard_s2", (R, c["ld"])), ("cate_s1", (CN, c["dc"])), ("cate_s2", (CN, c["dc"])))}
    lr = F32(OPT_LR[kind])
    out = twice(lambda: run_dense(c, sd, reg, kind, lr, slots0))
    _, b1, b2, eps = OPTIMIZERS[kind]
    ref_w, ref_c, ref_s, _ = sr.apply_dense(c["shard0"], c["cate0"], *ref_args(c), sd[0], sd[1], reg,
                                            opt=dict(kind=kind, lr=lr, b1=b1, b2=b2, eps=eps, step=3, **slots0))
    rec = {}
    for name, got, want, start in (("shard", out["shard"], ref_w, c["shard0"]), ("cate", out["cate"], ref_c, c["cate0"])):
        bound = 1e-5 * np.abs(want - d(start)).max() + 1e-7
        rec[name] = np.abs(d(got) - want).max() / bound
        assert rec[name] <= 1.0, (name, rec[name])
    for k in ("shard_s1", "shard_s2", "cate_s1", "cate_s2"):
        bound = 1e-5 * np.abs(ref_s[k]).max() + 1e-12
        rec[k] = np.abs(d(out[k]) - ref_s[k]).max() / bound
        assert rec[k] <= 1.0, (k, rec[k])
    record("apply_opt[%s-%s]" % (kind, GEOMETRY_IDS[GEOMETRY.index((G, wi, empty))]), **rec)
    for k, start in (("shard", c["shard0"]), ("shard_s1", slots0["shard_s1"]), ("shard_s2", slots0["shard_s2"])):
        assert same_bits(out[k][:, W:], start[:, W:]), k                      # [W, ld): bit for bit
    # item_b: column ri of the item rows
    still = np.ones(CI, bool)
    still[c["rows"][c["rows"] < CI]] = False                                  # not sent
    zero = np.zeros(CI, bool)
    zero[c["quiet"]] = True                                                   # sent, summed gradient exactly 0.0
    assert still.any() and zero.any() and (~still & ~zero).any() and (c["sum"][:CI, ri][zero] == 0.0).all()
    same = np.ones(CI, bool)
    for k, start in (("shard", c["shard0"]), ("shard_s1", slots0["shard_s1"]), ("shard_s2", slots0["shard_s2"])):
        same &= bits(out[k][:CI, ri]) == bits(start[:CI, ri])
    if kind == "adam":
        assert not same.any()
    else:
        assert same[still | zero].all() and not same[~still & ~zero].any()
    assert not out["slots"].any()
    check_sums(out["sq"], out["sq32"], (d(out["shard"][:, :W]) ** 2)[c["rg"]].sum(), (d(out["cate"]) ** 2).sum())


# ---------------------------------------------------------------------------------------------------------- C, D: lazy forms
STAMP = 77


def stale_slots(G, n, stamp, seed):
    """slots64 as earlier steps left them: (stamp - 1) << 32 | k with in-range k, a tenth under other stamps -> int64 [R * G]"""
    rng = np.random.RandomState(seed)
    hi = np.full(R * G, (stamp - 1) & 0xFFFFFFFF, np.uint64)
    other = rng.rand(R * G) < 0.1
    rnd = rng.randint(0, 2 ** 32, R * G, dtype=np.uint64)
    rnd[rnd == stamp] = stamp + 5
    hi[other] = rnd[other]
    lo = rng.randint(1, max(n, 1) + 1, R * G).astype(np.uint64)
    return ((hi << np.uint64(32)) | lo).view(np.int64)


class LazyState:
    """the device buffers one lazy owner update works on (fresh copies of a case's input)"""

    def __init__(self, c, sd, slots64):
        self.shard, self.cate = dev(c["shard0"]), dev(c["cate0"])
        self.g_cate, self.sd = dev(c["g_cate"]), dev(sd)
        self.slots64 = dev(slots64)
        self.sq = torch.tensor([5.0, 7.0], dtype=torch.float64, device="cuda")
        self.sq32 = torch.zeros(1, device="cuda")
        self.scale = torch.full((1,), 0.93, device="cuda")

    def out(self, **more):
        o = dict(shard=host(self.shard), cate=host(self.cate), sq=host(self.sq), sq32=host(self.sq32), scale=host(self.scale))
        o.update(more)
        return o


def run_lazy(c, st, stamp, rows=None, src_off=None, vals=None):
    L, lib = _lib()
    G, W = c["G"], c["W"]
    rows = c["rows"] if rows is None else rows
    src_off = c["src_off"] if src_off is None else src_off
    vals = c["vals"] if vals is None else vals
    n = len(rows)
    keep = [dev(vals), dev(rows)]
    nws = int(lib.tlsan_shard_apply_lazy_workspace(n, CN))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    L.check(lib.tlsan_shard_apply_lazy(st.shard.data_ptr(), c["ld"], CI, R, W, c["ri"], c["ru"], keep[0].data_ptr(), c["ldv"],
                                       keep[1].data_ptr(), n, (C.c_int32 * (G + 1))(*np.asarray(src_off).tolist()), G,
                                       st.slots64.data_ptr(), stamp, c["gscale"], st.sd.data_ptr(), st.cate.data_ptr(), CN, c["dc"],
                                       st.g_cate.data_ptr(), st.sq.data_ptr(), st.sq32.data_ptr(), st.scale.data_ptr(),
                                       ws.data_ptr(), nws, _stream()), "tlsan_shard_apply_lazy")
    torch.cuda.synchronize()


def check_lazy(c, sd, out, shard0, cate0, rows, src_off, vals, sq0, name):
    """one lazy update's output against the reference, from the tables shard0 / cate0 and the running sum sq0"""
    W, d = c["W"], np.float64
    ref_w, ref_c, P_new, _, _ = sr.apply_lazy(shard0, cate0, rows, src_off, vals, c["g_cate"], CI, W, c["ri"], c["ru"], c["gscale"], sd)
    acc, got = sr.source_sum(R, W, rows, src_off, vals)
    s = np.where(c["rg"], d(sd[2]), d(sd[0]))
    w0 = d(shard0[:, :W])
    S = np.abs(w0) + s * d(c["gscale"]) * np.abs(acc)
    err = np.abs(d(out["shard"][:, :W]) - ref_w[:, :W]) / (U * S)
    Sc = np.abs(d(cate0)) + d(sd[2]) * d(c["gscale"]) * np.abs(d(c["g_cate"]))
    errc = np.abs(d(out["cate"]) - ref_c) / (U * Sc)
    assert err[got].max() <= 8.0, (err[got].max(), np.unravel_index(err.argmax(), err.shape))
    assert errc.max() <= 8.0, errc.max()
    assert got.any() and not got.all()
    assert same_bits(out["shard"][~got], shard0[~got])                          # rows nobody sent: bit for bit, all ld columns
    assert same_bits(out["shard"][:, W:], shard0[:, W:])
    assert same_bits(out["shard"][:, :W][~c["lv"]], shard0[:, :W][~c["lv"]])   # [live, W)
    moved = (bits(out["shard"][:, :W]) != bits(shard0[:, :W]))
    assert moved[got][c["lv"][got]].mean() > 0.9
    assert bits(out["scale"])[0] == bits(np.array([sd[3]], F32))[0]
    delta = ((d(out["shard"][:, :W]) ** 2) - w0 ** 2)[c["rg"]].sum()
    worst = check_sums(out["sq"], out["sq32"], sq0 + delta, (d(out["cate"]) ** 2).sum())
    record(name, rows_uS=err[got].max(), cate_uS=errc.max(), sums_frac=worst)


def second_set(c):
    """the rows of a second step: source s sends what source s + 1 sent before (in part), so that the first step's marks name
    rows that a source does not send now"""
    G = c["G"]
    per = [c["per"][(s + 1) % G][1::2] for s in range(G)]
    if G == 1:
        per = [np.setdiff1d(np.arange(3, R, 7, dtype=np.int32), c["per"][0][:5])]
    rows = np.concatenate(per).astype(np.int32)
    src_off = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int32)
    rng = np.random.RandomState(9)
    vals = np.full((len(rows), c["ldv"]), np.nan, F32)
    vals[:, :c["W"]] = rng.randn(len(rows), c["W"]).astype(F32)
    live = np.where(rows < CI, c["ri"] + 1, c["ru"])
    vals[:, :c["W"]][np.arange(c["W"])[None, :] >= live[:, None]] = 0.0
    return rows, src_off, vals


_LAZY_RESULTS = {}


def lazy_result(G, wi, empty):
    """C's result for a geometry (computed once; D compares the static form with it)"""
    key = (G, wi, empty)
    if key not in _LAZY_RESULTS:
        c = received(G, wi, empty)
        sd, _, _ = step_dev_for(G, P=0.93)

        def run():
            st = LazyState(c, sd, stale_slots(G, c["n"], STAMP, 3))
            run_lazy(c, st, STAMP)
            return st.out()

        _LAZY_RESULTS[key] = (c, sd, twice(run))
    return _LAZY_RESULTS[key]


@pytest.mark.parametrize("G,wi,empty", GEOMETRY, ids=GEOMETRY_IDS)
def test_shard_apply_lazy(G, wi, empty):
    """C. tlsan_shard_apply_lazy over slots that hold the previous step's marks and marks of other stamps: received rows
    within 8 u S, everything else bit for bit, the scale committed, the running sums kept.  A second step on the same buffers
    under stamp + 1, whose sources send other rows than the marks of the first step name, moves its own rows only."""
    c, sd, out = lazy_result(G, wi, empty)
    name = GEOMETRY_IDS[GEOMETRY.index((G, wi, empty))]
    check_lazy(c, sd, out, c["shard0"], c["cate0"], c["rows"], c["src_off"], c["vals"], 5.0, "apply_lazy[%s]" % name)
    rows2, off2, vals2 = second_set(c)
    st = LazyState(c, sd, stale_slots(G, c["n"], STAMP, 3))
    run_lazy(c, st, STAMP)
    mid = st.out()
    assert same_bits(mid["shard"], out["shard"])
    run_lazy(c, st, STAMP + 1, rows2, off2, vals2)
    check_lazy(c, sd, st.out(), mid["shard"], mid["cate"], rows2, off2, vals2, mid["sq"][0], "apply_lazy_second[%s]" % name)


def run_lazy_static(c, st, stamp_value, cap, rows_s, vals_s, marked, recvbuf=None):
    """tlsan_shard_apply_lazy_static over G * cap slots; marked: the marks come from tlsan_shard_gather_static under the
    same device stamp (and the rows from its recv_rows) -> the device stamp afterwards"""
    L, lib = _lib()
    G, W = c["G"], c["W"]
    stamp = dev(np.array([stamp_value], np.uint32).view(np.int32))
    vals_d = dev(vals_s)
    if marked:
        rb = dev(recvbuf)
        rows_out = torch.full((G * cap, W), -5.0, device="cuda")
        rows_d = torch.full((G * cap,), -7, dtype=torch.int32, device="cuda")
        L.check(lib.tlsan_shard_gather_static(st.shard.data_ptr(), c["ld"], R, W, rb.data_ptr(), cap, G, rows_out.data_ptr(),
                                              rows_d.data_ptr(), st.slots64.data_ptr(), stamp.data_ptr(), _stream()),
                "tlsan_shard_gather_static")
        assert np.array_equal(host(rows_d), rows_s)
    else:
        rows_d = dev(rows_s)
    nws = int(lib.tlsan_shard_apply_lazy_workspace(G * cap, CN))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    L.check(lib.tlsan_shard_apply_lazy_static(st.shard.data_ptr(), c["ld"], CI, R, W, c["ri"], c["ru"], vals_d.data_ptr(), c["ldv"],
                                              rows_d.data_ptr(), cap, G, st.slots64.data_ptr(), stamp.data_ptr(), 1 if marked else 0,
                                              c["gscale"], st.sd.data_ptr(), st.cate.data_ptr(), CN, c["dc"], st.g_cate.data_ptr(),
                                              st.sq.data_ptr(), st.sq32.data_ptr(), st.scale.data_ptr(), ws.data_ptr(), nws,
                                              _stream()), "tlsan_shard_apply_lazy_static")
    return int(host(stamp).view(np.uint32)[0])


@pytest.mark.parametrize("G,wi,empty", GEOMETRY, ids=GEOMETRY_IDS)
def test_shard_apply_lazy_static(G, wi, empty):
    """D. C's input laid into G x cap slots (empty slots: row -1, NaN gradients): the marks written by the call itself, or
    by tlsan_shard_gather_static under the same device stamp, give C's tables and scale bit for bit and its sums to 1e-9;
    the device stamp advances by one, and the successor of 2^32 - 2 is 1 (include/tlsan.h: stamps run 1 .. 2^32 - 2)."""
    c, sd, want = lazy_result(G, wi, empty)
    counts = [len(x) for x in c["per"]]
    cap = max(counts) + 3
    rows_s = np.full(G * cap, -1, np.int32)
    vals_s = np.full((G * cap, c["ldv"]), np.nan, F32)
    recvbuf = np.full((G, 1 + cap), -1, np.int32)
    for s in range(G):
        rows_s[s * cap:s * cap + counts[s]] = c["per"][s]
        vals_s[s * cap:s * cap + counts[s]] = c["vals"][c["src_off"][s]:c["src_off"][s + 1]]
        recvbuf[s, 0] = counts[s]
        recvbuf[s, 1:1 + counts[s]] = c["per"][s]
    for stamp0, marked, slots in ((STAMP, 0, stale_slots(G, G * cap, STAMP, 3)), (STAMP, 1, stale_slots(G, G * cap, STAMP, 4)),
                                  (0xFFFFFFFE, 0, np.zeros(R * G, np.int64))):
        def run():
            st = LazyState(c, sd, slots)
            after = run_lazy_static(c, st, stamp0, cap, rows_s, vals_s, marked, recvbuf)
            return st.out(stamp=np.array([after], np.int64))

        out = twice(run)
        for k in ("shard", "cate", "scale"):
            assert same_bits(out[k], want[k]), (k, stamp0, marked)
        for j in range(2):
            assert abs(out["sq"][j] - want["sq"][j]) <= 1e-9 * max(1.0, abs(want["sq"][j])), (j, stamp0, marked)
        assert out["sq32"][0] == np.float32(out["sq"][0])
        assert out["stamp"][0] == (1 if stamp0 == 0xFFFFFFFE else stamp0 + 1), (stamp0, out["stamp"][0])


# ---------------------------------------------------------------------------------------------------------- E, F: gathers
@pytest.mark.parametrize("G", [1, 5, 16])
def test_shard_gather(G):
    """E. tlsan_shard_gather: the requested rows of shard [R, ld] in source order, their numbers, nothing past n_recv * W"""
    L, lib = _lib()
    W = 76
    ld = W + 4
    rng = np.random.RandomState(40 + G)
    counts = rng.randint(1, 30, G)
    if G > 1:
        counts[1] = 0
        counts[G - 1] = 0 if G == 16 else counts[G - 1]
    per = [np.sort(rng.choice(R, k, replace=False)).astype(np.int32) for k in counts]
    per[0] = np.unique(np.concatenate([per[0], [0, R - 1]])).astype(np.int32)
    counts = [len(x) for x in per]
    cap = max(counts) + 2
    recvbuf = np.full((G, 1 + cap), -1, np.int32)
    for s in range(G):
        recvbuf[s, 0] = counts[s]
        recvbuf[s, 1:1 + counts[s]] = per[s]
    rows = np.concatenate(per)
    n = len(rows)
    shard0 = rng.randn(R, ld).astype(F32)

    def run():
        shard, rb = dev(shard0), dev(recvbuf)
        rows_out = torch.full(((n + 3) * W,), -5.0, device="cuda")
        recv_rows = torch.full((n + 3,), -9, dtype=torch.int32, device="cuda")
        L.check(lib.tlsan_shard_gather(shard.data_ptr(), ld, R, W, rb.data_ptr(), cap, G, n, rows_out.data_ptr(), recv_rows.data_ptr(),
                                       _stream()), "tlsan_shard_gather")
        return dict(rows_out=host(rows_out), recv_rows=host(recv_rows))

    out = twice(run)
    assert 0 in counts[1:] or G == 1
    assert same_bits(out["rows_out"][:n * W].reshape(n, W), np.ascontiguousarray(shard0[rows, :W]))
    assert (out["rows_out"][n * W:] == -5.0).all()
    assert np.array_equal(out["recv_rows"][:n], rows) and (out["recv_rows"][n:] == -9).all()


@pytest.mark.parametrize("d_emb,tail", [(32, 10), (64, 1), (128, 90)])
def test_shard_gather_wire_bf16(d_emb, tail):
    """F. tlsan_shard_gather_wire_bf16: per slot [d_emb bf16, round to nearest even | tail fp32 | pad], a pitch 16 bytes
    larger than needed; ties, their neighbours, signed zeros, infinities and the largest finite fp32 planted in requested rows.
    Pad bytes and empty slots keep their 0xA5; recv_rows and the slot marks as tlsan_shard_gather_static leaves them."""
    L, lib = _lib()
    G, cap, stamp_v = 4, 24, 9
    ld = (d_emb + tail + 3) // 4 * 4 + 4
    pitch = (2 * d_emb + 4 * tail + 15) // 16 * 16 + 16
    rng = np.random.RandomState(d_emb + tail)
    counts = [24, 0, 17, 9]
    per = [np.sort(rng.choice(R, k, replace=False)).astype(np.int32) for k in counts]
    per[2][0], per[2][-1] = 0, R - 1
    per[2] = np.unique(per[2]).astype(np.int32)
    counts = [len(x) for x in per]
    assert any(r < CI for r in per[0]) and any(r >= CI for r in per[0])         # item rows and user rows
    shard0 = rng.randn(R, ld).astype(F32)
    planted = np.array([b for b, _ in sr.BF16_PLANTED], np.uint32).view(F32)
    for k, r in enumerate(per[0][:6].tolist() + per[3][:3].tolist()):           # known places in requested rows
        cols = (np.arange(len(planted)) * 3 + k) % d_emb
        shard0[r, cols] = planted
    assert np.isfinite(shard0).sum() < shard0.size and not np.isnan(shard0).any()
    recvbuf = np.full((G, 1 + cap), -1, np.int32)
    for s in range(G):
        recvbuf[s, 0] = counts[s]
        recvbuf[s, 1:1 + counts[s]] = per[s]

    def run():
        shard, rb = dev(shard0), dev(recvbuf)
        wire = torch.full((G * cap * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
        recv_rows = torch.full((G * cap,), -9, dtype=torch.int32, device="cuda")
        slots = torch.zeros(R * G, dtype=torch.int64, device="cuda")
        stamp = torch.full((1,), stamp_v, dtype=torch.int32, device="cuda")
        L.check(lib.tlsan_shard_gather_wire_bf16(shard.data_ptr(), ld, R, d_emb, tail, rb.data_ptr(), cap, G, wire.data_ptr(), pitch,
                                                 recv_rows.data_ptr(), slots.data_ptr(), stamp.data_ptr(), _stream()),
                "tlsan_shard_gather_wire_bf16")
        return dict(wire=host(wire), recv_rows=host(recv_rows), slots=host(slots), stamp=host(stamp))

    out = twice(run)
    wire = out["wire"].reshape(G, cap, pitch)
    rr, sl = out["recv_rows"].reshape(G, cap), out["slots"].reshape(R, G)
    seen = set()
    for s in range(G):
        k = counts[s]
        assert np.array_equal(rr[s, :k], per[s]) and (rr[s, k:] == -1).all()
        assert (wire[s, k:] == 0xA5).all()                                           # empty slots
        rows = shard0[per[s]]
        half = np.ascontiguousarray(wire[s, :k, :2 * d_emb]).view(np.uint16)
        want = sr.bf16_rne_bits(rows[:, :d_emb])
        assert np.array_equal(half, want), (s, np.argwhere(half != want)[:4])
        seen |= set(want.ravel().tolist())
        fl = np.ascontiguousarray(wire[s, :k, 2 * d_emb:2 * d_emb + 4 * tail]).view(np.uint32)
        assert np.array_equal(fl, bits(np.ascontiguousarray(rows[:, d_emb:d_emb + tail])))
        assert (wire[s, :k, 2 * d_emb + 4 * tail:] == 0xA5).all()                    # pad bytes
        for j in range(k):
            assert sl[per[s][j], s] == (stamp_v << 32) | (s * cap + j + 1)
    assert {h for _, h in sr.BF16_PLANTED} <= seen
    assert np.count_nonzero(sl) == sum(counts) and out["stamp"][0] == stamp_v


# ---------------------------------------------------------------------------------------------------------- G: summary
def summary_problem(G, regime, kind):
    L, lib = _lib()
    cfg = make_config(d=64)
    dims = L.Dims(cfg["user_count"], cfg["item_count"], cfg["cate_count"], cfg["hidden_units"], cfg["itemid_embedding_size"],
                  cfg["cateid_embedding_size"], cfg["num_heads"], cfg["Ls"])
    lay = L.DenseLayout()
    L.check(lib.tlsan_dense_layout_of(C.byref(dims), C.byref(lay)), "tlsan_dense_layout_of")
    n_dense, n_cate, D = lay.n_dense, 7 * 32, 64
    assert lay.k0 - lay.K == D * D
    rng = np.random.RandomState(10 * G + len(regime) + len(kind))
    flat = np.zeros(n_dense + n_cate + 8, F32)
    flat[:n_dense + n_cate] = (0.05 * G * rng.randn(n_dense + n_cate)).astype(F32)
    flat[n_dense + n_cate:n_dense + n_cate + 3] = np.array([0.69 * G, 2.5 * G * G, 310.0], F32)
    lr, reg, S_cate = F32({"sgd": 0.7}.get(kind, OPT_LR.get(kind, 0.0))), F32(1e-2), 41.5
    P = F32(0.93) if regime == "scale" else None
    free = sr.summary(flat, n_dense, n_cate, G, lr, reg, F32(1e30), S_cate, P=P)
    clip = F32((2.0 if regime == "unclipped" else 0.37) * free["norm"])
    dense0 = rng.uniform(-0.7, 0.7, n_dense).astype(F32)
    s1 = rng.uniform(1e-3, 2e-3, n_dense).astype(F32)
    s2 = rng.uniform(1e-3, 2e-3, n_dense).astype(F32)
    return dict(L=L, lib=lib, dims=dims, lay=lay, n_dense=n_dense, n_cate=n_cate, D=D, flat=flat, lr=lr, reg=reg, clip=clip,
                S_cate=S_cate, P=P, dense0=dense0, s1=s1, s2=s2, G=G, kind=kind)


def run_summary(p, plain=False, scale_with_kind=None):
    """tlsan_shard_summary_opt (plain: tlsan_shard_summary) on fresh copies -> (return code, dict of host arrays)"""
    from tlsan_amd.model import OPTIMIZERS
    L, lib = p["L"], p["lib"]
    flat, dense = dev(p["flat"]), dev(p["dense0"])
    kt = torch.full((p["D"] * p["D"],), -5.0, device="cuda")
    sc = torch.tensor([p["S_cate"]], dtype=torch.float64, device="cuda")
    step_dev = dev(np.array([9.0, 9.0, -3.5, -4.5], F32))
    loss, gnorm = torch.full((1,), -1.0, device="cuda"), torch.full((1,), -1.0, device="cuda")
    s1, s2 = dev(p["s1"]), dev(p["s2"])
    scale = dev(np.array([0.93 if p["P"] is None else p["P"]], F32))
    kind = scale_with_kind or p["kind"]
    code, b1, b2, eps = OPTIMIZERS[kind]
    use_scale = p["P"] is not None or scale_with_kind is not None
    opt = L.ShardOptimizer(code, 3, b1, b2, eps, s1.data_ptr(), s2.data_ptr(), s1.data_ptr(), s2.data_ptr(), s1.data_ptr(), s2.data_ptr(),
                           scale.data_ptr() if use_scale else None)
    head = (flat.data_ptr(), p["n_dense"], p["n_cate"], p["G"], p["lr"], p["reg"], p["clip"], sc.data_ptr(), dense.data_ptr(),
            kt.data_ptr(), C.byref(p["dims"]), step_dev.data_ptr(), loss.data_ptr(), gnorm.data_ptr())
    if plain:
        rc = lib.tlsan_shard_summary(*head, _stream())
    else:
        rc = lib.tlsan_shard_summary_opt(*head, C.byref(opt) if (kind != "sgd" or use_scale) else None, _stream())
    return rc, dict(flat=host(flat), dense=host(dense), kt=host(kt), step_dev=host(step_dev), loss=host(loss), gnorm=host(gnorm),
                    s1=host(s1), s2=host(s2), scale=host(scale))


SUMMARY_CASES = [(G, regime, kind) for G in (1, 3, 16) for regime, kinds in
                 (("unclipped", ("sgd", "adam", "rmsprop", "adadelta")), ("clipped", ("sgd", "adam", "rmsprop", "adadelta")),
                  ("scale", ("sgd",))) for kind in kinds]


@pytest.mark.parametrize("G,regime,kind", SUMMARY_CASES)
def test_shard_summary(G, regime, kind):
    """G. tlsan_shard_summary_opt: norm, step_dev[0..3], loss within 16 u; the dense weights within 8 u S (SGD) or the
    optimizer bounds; dense_KT the transposed K block of the new weights bit for bit; step_dev[2..3] and flat untouched."""
    from tlsan_amd.model import OPTIMIZERS
    p = summary_problem(G, regime, kind)
    d = np.float64
    _, b1, b2, eps = OPTIMIZERS[kind]
    ref = sr.summary(p["flat"], p["n_dense"], p["n_cate"], G, p["lr"], p["reg"], p["clip"], p["S_cate"], P=p["P"], dense=p["dense0"],
                     opt=dict(kind=kind, b1=b1, b2=b2, eps=eps, step=3, dense_s1=p["s1"], dense_s2=p["s2"]))
    assert abs(ref["norm"] - d(p["clip"])) > 1e-3 * d(p["clip"]) and (ref["coef"] < 1.0) == (regime != "unclipped")

    def run():
        rc, out = run_summary(p)
        assert rc == 0, p["lib"].tlsan_last_error()
        return out

    out = twice(run)
    rec = dict(gnorm=abs(d(out["gnorm"][0]) - ref["norm"]) / (U * ref["norm"]),
               loss=abs(d(out["loss"][0]) - ref["loss"]) / (U * ref["loss_scale"]))
    for j, v in enumerate(ref["step_dev"]):
        rec["step_dev%d" % j] = abs(d(out["step_dev"][j]) - v) / (U * abs(v))
    if p["P"] is None:
        assert same_bits(out["step_dev"][2:], np.array([-3.5, -4.5], F32))
    assert same_bits(out["scale"], np.array([0.93], F32))                      # (the scale is committed by the apply)
    assert same_bits(out["flat"], p["flat"])
    gd = np.abs(d(p["flat"][:p["n_dense"]])) / G
    if kind == "sgd":
        S = np.abs(d(p["dense0"])) + ref["step"] * gd
        rec["dense_uS"] = (np.abs(d(out["dense"]) - ref["dense"]) / (U * S)).max()
        assert same_bits(out["s1"], p["s1"]) and same_bits(out["s2"], p["s2"])
    else:
        rec["dense_frac"] = np.abs(d(out["dense"]) - ref["dense"]).max() / (1e-5 * np.abs(ref["dense"] - d(p["dense0"])).max() + 1e-7)
        for k in ("s1", "s2"):
            rec[k + "_frac"] = np.abs(d(out[k]) - ref["dense_" + k]).max() / (1e-5 * np.abs(ref["dense_" + k]).max() + 1e-12)
    record("summary[G%d-%s-%s]" % (G, regime, kind), **rec)
    for k in ("gnorm", "loss", "step_dev0", "step_dev1", "step_dev2", "step_dev3"):
        assert rec.get(k, 0.0) <= 16.0, (k, rec[k])
    assert rec.get("dense_uS", 0.0) <= 8.0, rec["dense_uS"]
    for k in ("dense_frac", "s1_frac", "s2_frac"):
        assert rec.get(k, 0.0) <= 1.0, (k, rec[k])
    K = out["dense"][p["lay"].K:p["lay"].k0].reshape(p["D"], p["D"])
    assert same_bits(out["kt"].reshape(p["D"], p["D"]), np.ascontiguousarray(K.T))
    if kind == "sgd" and p["P"] is None:          # the call without `opt` is the call with opt = NULL
        rc, plain = run_summary(p, plain=True)
        assert rc == 0
        for k in out:
            assert same_bits(plain[k], out[k]), k


def test_shard_summary_refuses_an_optimizer_with_a_scale():
    p = summary_problem(3, "clipped", "sgd")
    rc, out = run_summary(p, scale_with_kind="adam")
    assert rc == E_UNSUPPORTED
    assert same_bits(out["dense"], p["dense0"]) and same_bits(out["step_dev"], np.array([9.0, 9.0, -3.5, -4.5], F32))
    assert out["loss"][0] == -1.0 and (out["kt"] == -5.0).all()


# ---------------------------------------------------------------------------------------------------------- H: scan
@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 3 * 4096 + 5])
@pytest.mark.parametrize("ends", ["nonzero-nonzero", "zero-zero", "nonzero-zero"])
def test_scan_compact(n, ends):
    """H. tlsan_scan_compact: counts in 0..3 with long runs of zeros on both sides of the 4096-count chunks"""
    L, lib = _lib()
    rng = np.random.RandomState(n % 1000 + len(ends))
    cnt = rng.randint(0, 4, n).astype(np.int32)
    for _ in range(max(1, n // 700)):                       # long zero runs
        a = rng.randint(0, n)
        cnt[a:a + rng.randint(50, 600)] = 0
    first, last = ends.split("-")
    cnt[0] = 2 if first == "nonzero" else 0
    cnt[-1] = 3 if last == "nonzero" else 0                 # (n = 1: the last element decides)
    want_prefix = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    want_uniq = np.nonzero(cnt)[0].astype(np.int32)

    def run(with_uniq=True):
        cd = dev(cnt)
        prefix = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
        uniq = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
        nu = torch.full((1,), -9, dtype=torch.int32, device="cuda")
        L.check(lib.tlsan_scan_compact(cd.data_ptr(), n, prefix.data_ptr(), uniq.data_ptr() if with_uniq else None,
                                       nu.data_ptr() if with_uniq else None, _stream()), "tlsan_scan_compact")
        return dict(prefix=host(prefix), uniq=host(uniq), nu=host(nu), cnt=host(cd))

    out = twice(run)
    assert np.array_equal(out["prefix"][:n], want_prefix) and (out["prefix"][n:] == -9).all()
    assert out["nu"][0] == len(want_uniq)
    assert np.array_equal(out["uniq"][:len(want_uniq)], want_uniq) and (out["uniq"][len(want_uniq):] == -9).all()
    assert np.array_equal(out["cnt"], cnt)
    bare = run(with_uniq=False)
    assert np.array_equal(bare["prefix"], out["prefix"]) and (bare["uniq"] == -9).all() and bare["nu"][0] == -9


# ---------------------------------------------------------------------------------------------------------- I: refusals
def test_refusals_leave_the_shard_alone():
    """I. What the owner updates refuse, with the error code include/tlsan.h gives it, before anything is launched: the
    shard keeps its bits."""
    L, lib = _lib()
    G, (ri, ru, W, dc) = 3, WIDTHS[1]
    c = received(3, 1, 0)
    sd, _, reg = step_dev_for(G, P=0.93)
    big = 264                                                   # room for W = 260 rows
    shard0 = np.random.RandomState(2).uniform(-0.8, 0.8, (R, big)).astype(F32)
    shard = dev(shard0)
    cate, g_cate, sdd = dev(c["cate0"]), dev(c["g_cate"]), dev(sd)
    vals = torch.zeros(c["n"], big, device="cuda")
    rows = dev(c["rows"])
    slots = torch.zeros(R * 17, dtype=torch.int64, device="cuda")
    sq = torch.zeros(2, dtype=torch.float64, device="cuda")
    scale = torch.ones(1, device="cuda")
    nws = int(lib.tlsan_shard_apply_workspace(R, CN))
    nlw = int(lib.tlsan_shard_apply_lazy_workspace(c["n"], CN))
    ws = torch.empty(max(nws, nlw) + 64, dtype=torch.uint8, device="cuda")

    def off(G, last=None):
        o = np.linspace(0, c["n"], G + 1).astype(np.int32)
        if last is not None:
            o[-1] = last
        return (C.c_int32 * (G + 1))(*o.tolist())

    def dense(G=G, W=W, so=None, ws_bytes=nws):
        return lib.tlsan_shard_apply(shard.data_ptr(), big, CI, R, W, min(ri, W), min(ru, W), vals.data_ptr(), big, rows.data_ptr(),
                                     c["n"], so or off(G), G, slots.data_ptr(), F32(1.0 / G), sdd.data_ptr(), reg, cate.data_ptr(), CN, dc,
                                     g_cate.data_ptr(), sq.data_ptr(), None, ws.data_ptr(), ws_bytes, _stream())

    def lazy(G=G, W=W, so=None, stamp=5, ws_bytes=nlw):
        return lib.tlsan_shard_apply_lazy(shard.data_ptr(), big, CI, R, W, min(ri, W), min(ru, W), vals.data_ptr(), big, rows.data_ptr(),
                                          c["n"], so or off(G), G, slots.data_ptr(), stamp, F32(1.0 / G), sdd.data_ptr(), cate.data_ptr(),
                                          CN, dc, g_cate.data_ptr(), sq.data_ptr(), None, scale.data_ptr(), ws.data_ptr(), ws_bytes,
                                          _stream())

    for what, rc, want in (("dense, G = 17", dense(G=17), E_UNSUPPORTED), ("lazy, G = 17", lazy(G=17), E_UNSUPPORTED),
                           ("dense, W = 260", dense(W=260), E_UNSUPPORTED),
                           ("dense, W = 42", dense(W=42), E_UNSUPPORTED), ("lazy, W = 42", lazy(W=42), E_UNSUPPORTED),
                           ("dense, src_off short", dense(so=off(G, c["n"] - 1)), E_BADARG),
                           ("lazy, src_off short", lazy(so=off(G, c["n"] - 1)), E_BADARG),
                           ("lazy, stamp = 0", lazy(stamp=0), E_UNSUPPORTED),
                           ("dense, workspace one byte short", dense(ws_bytes=nws - 1), E_WORKSPACE),
                           ("lazy, workspace one byte short", lazy(ws_bytes=nlw - 1), E_WORKSPACE)):
        assert rc == want, (what, rc, lib.tlsan_last_error())
    assert same_bits(host(shard), shard0) and same_bits(host(cate), c["cate0"])
    assert not host(slots).any() and host(scale)[0] == 1.0 and not host(sq).any()

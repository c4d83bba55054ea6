"""A batch's destination index (csrc/tlsan_index.h), product by product against numpy (tests/index_ref.py): use counts,
segment offsets, cursors, used-row records, hot rows, the ranking of the batch, the per-category sample lists -- in every form
tlsan_batch_index builds them (tests/index_cases.py), exactly: the index is integer work and a fixed function of the batch.
Each case builds ONE index into a poisoned slot of a fresh state and reads it back through tlsan_index_layout_of; nothing
consumes these indexes.  The persistent counters' contract (zero at rest) is checked after real training steps."""
import ctypes as C

import numpy as np
import pytest

from tests import index_ref as R
from tests.helpers import batch_tuple, make_config, random_batch
from tests.index_cases import AP_HOT, AP_HOT_CAP, BY_NAME, CASES, LAZY, PLAN_FIELDS

pytestmark = pytest.mark.gpu

POISON = -0x2152ABCD      # no valid position, id, count or sample
TABLES = (("item", 1), ("uc", 2), ("user", 4))      # (name, its bit of tlsan_index_plan.sparse)
COUNTERS = ("cnt_item", "cnt_uc", "cnt_user", "flag_user")


def _layout(m, slot):
    from tlsan_amd import _lib as L
    lay = L.IndexLayout()
    L.check(m.lib.tlsan_index_layout_of(C.byref(m.dims), slot, C.byref(lay)), "tlsan_index_layout_of")
    assert (lay.ap_hot, lay.ap_hot_cap) == (AP_HOT, AP_HOT_CAP)
    return lay


def _plan(m, B, Sn, flags):
    from tlsan_amd import _lib as L
    plan = L.IndexPlan()
    L.check(m.lib.tlsan_index_plan_of(C.byref(m.dims), B, Sn, flags, C.byref(plan)), "tlsan_index_plan_of")
    return {f: getattr(plan, f) for f in PLAN_FIELDS}


def _views(m, slot):
    """the slot's arrays as int32 views of the model's own state tensor (tlsan_index_layout_of: byte offsets)"""
    import torch
    from tlsan_amd import _lib as L
    lay = _layout(m, slot)
    U, I, Cn = m.dims.user_count, m.dims.item_count, m.dims.cate_count
    s32 = m._state.view(torch.int32)
    size = dict(cnt_item=I, cnt_uc=Cn, cnt_user=U, off_item=I + 1, off_uc=Cn + 1, off_user=U + 1, cur_item=I, cur_uc=Cn,
                cur_user=U, urec_item=4 * I, urec_user=4 * U, perm=lay.rank_cap, uc_list=lay.uc_list_cap, hot_list=lay.ap_hot_cap,
                flag_user=(U + 255) // 256, scan_ticket=L.INDEX_SLOTS, n_uniq=2, n_hot=1)
    out = {}
    for name, n in size.items():
        off = getattr(lay, name)
        assert off % 4 == 0 and 0 <= off and off + 4 * n <= m._state.numel(), name
        out[name] = s32[off // 4: off // 4 + n]
    return out


PRODUCTS = ("off_item", "off_uc", "off_user", "cur_item", "cur_uc", "cur_user", "urec_item", "urec_user", "perm", "uc_list", "hot_list")


def _build(m, db, slot, flags, poison=True):
    """one tlsan_batch_index into `slot`; returns the slot's arrays on the host"""
    import torch
    from tlsan_amd import _lib as L
    v = _views(m, slot)
    if poison:
        for name in PRODUCTS:
            v[name].fill_(POISON)
    L.check(m.lib.tlsan_batch_index(C.byref(m.dims), C.byref(db.c), m.cparams.item_cate, m._state.data_ptr(), slot | flags,
                                    m._stream()), "tlsan_batch_index")
    torch.cuda.synchronize(m.device)
    return _read(m, slot)


def _read(m, slot):
    return {k: t.cpu().numpy().astype(np.int64) for k, t in _views(m, slot).items()}


def _fresh(case):
    from tlsan_amd.model import Model
    cfg = make_config(**case.cfg)
    b, cat = case.batch(cfg)
    m = Model(cfg, cat)
    return cfg, b, cat, m, m.device_batch(batch_tuple(b))


def _check(got, ref, plan, U, I, Cn, B):
    """every product of one built slot against the reference"""
    for (name, bit), n, sorted_side in zip(TABLES, (I, Cn, U), (plan["isort"], 0, plan["usort"])):
        t = ref["cate" if name == "uc" else name]
        cnt, off, cur = got["cnt_" + name], got["off_" + name], got["cur_" + name]
        # a side that is sorted has no counters; one that is counted holds the uses until a step counts them back
        assert np.array_equal(cnt, np.zeros(n, np.int64) if sorted_side else t["cnt"]), name
        want_cur = t["off"][:n]
        if name == "uc" and plan["uc_list"]:
            want_cur = t["off"][1:]            # k_uc_fill drew every category's positions
        if plan["sparse"] & bit:               # written for the used rows only
            used = t["rec"][:, 0]
            rest = np.ones(n, bool)
            rest[used] = False
            assert np.array_equal(off[used], t["off"][used]) and np.array_equal(cur[used], want_cur[used]), name
            assert off[n] == t["off"][n], name
            assert (off[:n][rest] == POISON).all() and (cur[rest] == POISON).all(), name
        else:
            assert np.array_equal(off, t["off"]), name
            assert np.array_equal(cur, want_cur), name
        if name != "uc":
            k = 0 if name == "item" else 1
            assert got["n_uniq"][k] == t["n_uniq"], name
            rec = got["urec_" + name].reshape(-1, 4)
            assert np.array_equal(rec[:t["n_uniq"]], t["rec"]), name
            assert (rec[t["n_uniq"]:] == POISON).all(), name
    # hot rows: their number always; the list (record slots) as a set while it holds them all -- its order is the atomics'
    n_hot = int(got["n_hot"][0])
    assert n_hot == len(ref["hot"])
    if n_hot <= AP_HOT_CAP:
        assert set(got["hot_list"][:n_hot].tolist()) == ref["hot"] and len(ref["hot"]) == n_hot
        assert (got["hot_list"][n_hot:] == POISON).all()
    # the ranking
    if plan["rank"]:
        G = (B + 15) // 16
        assert np.array_equal(got["perm"][:16 * G], ref["perm"])
        assert (got["perm"][16 * G:] == POISON).all()
    else:
        assert (got["perm"] == POISON).all()
    # the samples of every category: sets (the order inside a category is the atomics' when several blocks fill it)
    if plan["uc_list"]:
        off = ref["cate"]["off"]
        for c in range(Cn):
            seg = got["uc_list"][off[c]:off[c + 1]].tolist()
            assert len(seg) == len(ref["lists"][c]) and set(seg) == ref["lists"][c], c
        assert (got["uc_list"][B:] == POISON).all()
    else:
        assert (got["uc_list"] == POISON).all()
    assert not got["flag_user"].any() and not got["scan_ticket"].any()      # zero after the scan


def _canon(got, Cn):
    """a built slot with its two order freedoms taken out: the hot list and every category's list sorted"""
    out = dict(got)
    n_hot = int(got["n_hot"][0])
    out["hot_list"] = np.sort(got["hot_list"][:min(n_hot, AP_HOT_CAP)]) if n_hot <= AP_HOT_CAP else np.zeros(0, np.int64)
    lst = got["uc_list"].copy()
    if (lst != POISON).any():
        off = got["off_uc"]
        for c in range(Cn):
            lst[off[c]:off[c + 1]] = np.sort(lst[off[c]:off[c + 1]])
    out["uc_list"] = lst
    return out


def _same(a, b, Cn):
    a, b = _canon(a, Cn), _canon(b, Cn)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_index_products(name):
    case = BY_NAME[name]
    cfg, b, cat, m, db = _fresh(case)
    U, I, Cn = cfg["user_count"], cfg["item_count"], cfg["cate_count"]
    plan = _plan(m, case.B, case.Sn, case.flags)
    assert plan == case.plan          # the case takes the form it was written for
    ref = R.build(b, U, I, Cn, cfg["Ls"], cat, cseg=bool(plan["cseg"]), rank=bool(plan["rank"]), by_window=plan["by_window"],
                  ap_hot=AP_HOT)
    got = _build(m, db, 0, case.flags)
    _check(got, ref, plan, U, I, Cn, case.B)
    # determinism: a second build on a fresh state has the same bits (but for the two order freedoms)
    _, _, _, m2, db2 = _fresh(case)
    _same(got, _build(m2, db2, 0, case.flags), Cn)


@pytest.mark.parametrize("name", ["counted-lazy", "isort-usort-lazy", "uclist-600-shared", "rank-Ls33-B250"])
def test_slots_are_independent(name):
    """the same batch built into slots 0, 1 and 2 of one state gives the same bits; another batch built into slot 1 leaves
    slot 0's products untouched"""
    case = BY_NAME[name]
    cfg, b, cat, m, db = _fresh(case)
    Cn = cfg["cate_count"]
    got = [_build(m, db, k, case.flags) for k in range(3)]
    for k in (1, 2):
        _same(got[0], got[k], Cn)
    before = _read(m, 0)
    b2, _ = random_batch(cfg, B=case.B, Sn=case.Sn, seed=999)
    other = _build(m, m.device_batch(batch_tuple(b2)), 1, case.flags, poison=False)
    after = _read(m, 0)
    for k in before:
        if k != "scan_ticket":          # (shared by the slots; zero either way, see below)
            assert np.array_equal(before[k], after[k]), k
    assert not after["scan_ticket"].any()
    assert not np.array_equal(other["off_item"], got[1]["off_item"])        # (slot 1 did take the other batch)


# ---- zero at rest: tlsan_batch_index only ADDS to the persistent counters, the consuming step counts them back
_REST = [   # (the case whose shape is trained, l2 modes)
    ("counted", ("dense", "lazy")), ("scan-16-chunks+1", ("dense", "lazy")), ("cseg-counted", ("dense", "lazy")),
    ("uclist-97-listed", ("dense", "lazy")), ("rank-Ls33-B33", ("dense", "lazy")),
    ("flags-one-piece-lazy", ("lazy",)), ("usort-65536-B1025-lazy", ("lazy",)), ("isort-65536-1blk-lazy", ("lazy",)),
    ("isort-usort-lazy", ("lazy",)),
]


def _counters_at_rest(m, what):
    import torch
    torch.cuda.synchronize(m.device)
    for slot in range(3):
        v = _views(m, slot)
        for name in COUNTERS + ("scan_ticket",):
            assert not bool(v[name].any().item()), (what, slot, name)


@pytest.mark.parametrize("name,l2", [(n, l2) for n, modes in _REST for l2 in modes])
def test_counters_are_zero_at_rest(name, l2):
    from tlsan_amd.model import Model
    case = BY_NAME[name]
    cfg = make_config(**case.cfg)
    _, cat = case.batch(cfg)
    m = Model(cfg, cat, l2_mode=l2)
    plan = _plan(m, case.B, case.Sn, LAZY if l2 == "lazy" else 0)
    for f in ("cseg", "uc_list", "usort", "isort", "two_level", "rank", "by_window"):        # the form the shape was chosen for
        assert plan[f] == case.plan[f], f
    dbs = [m.device_batch(batch_tuple(random_batch(cfg, B=case.B, Sn=case.Sn, seed=300 + s)[0])) for s in range(6)]
    # four steps, indexes built one and two steps ahead: all three slots cycle; the last two steps announce nothing
    m.train_async(dbs[0], 0.5, next_batch=dbs[1], after_next=dbs[2])
    m.train_async(dbs[1], 0.5, next_batch=dbs[2], after_next=dbs[3])
    m.train_async(dbs[2], 0.5)
    m.train_async(dbs[3], 0.5)
    _counters_at_rest(m, "four steps")
    m.grads(dbs[4])
    _counters_at_rest(m, "grads")
    if l2 == "lazy":        # a clipped step (the two-launch form owes a correction), then one more step
        clip = m.config["max_gradient_norm"]
        m.config["max_gradient_norm"] = 0.02
        m.train_async(dbs[4], 0.5, next_batch=dbs[5])
        assert m.last_gnorm() > 0.02          # (the step was clipped)
        m.config["max_gradient_norm"] = clip
        m.train_async(dbs[5], 0.5)
        _counters_at_rest(m, "clipped step")
        assert np.isfinite(float(m._out[0].item()))

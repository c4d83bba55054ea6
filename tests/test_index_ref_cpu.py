"""The numpy reference of a batch's destination index (tests/index_ref.py) against a brute-force construction -- a dict of
lists filled use by use, a sort by key written out -- and against its own invariants, on random and adversarial batches."""
import numpy as np
import pytest

from tests import index_ref as R
from tests.helpers import make_config, random_batch


def _batches():
    out = []
    for seed, (U, I, C, Ls, B, Sn) in enumerate([(50, 40, 7, 10, 37, 3), (50, 40, 7, 10, 1, 0), (1, 40, 7, 10, 20, 2),
                                                 (300, 5000, 2048, 10, 130, 4), (9, 3, 2, 33, 250, 5), (70, 90, 3, 10, 97, 0)]):
        cfg = make_config(U=U, I=I, C=C, Ls=Ls)
        b, cat = random_batch(cfg, B=B, Sn=Sn, seed=seed)
        out.append((cfg, b, cat))
    # adversarial: one item everywhere (a hot row), every length at its cap, lengths beyond the arrays' widths
    cfg = make_config(U=20, I=30, C=5, Ls=10)
    b, cat = random_batch(cfg, B=64, Sn=4, seed=77, full=True)
    for k in ("hist_i", "hist_i_new", "i"):
        b[k][:] = 29
    b["u"][:] = 19
    out.append((cfg, b, cat))
    b, cat = random_batch(cfg, B=33, Sn=4, seed=78)
    b["sl"] = b["sl"] + 100          # (clamped to Ls: the whole window is used, padding zeros included)
    b["sl_new"] = b["sl_new"] + 100
    out.append((cfg, b, cat))
    return out


def _brute(b, Ls, item_cate, cseg):
    """use by use: table -> {row: [use, ...]}"""
    rows = dict(item={}, user={}, cate={})
    B = len(b["u"])
    Sn = np.asarray(b["hist_i_new"]).reshape(B, -1).shape[1]
    n = 0
    for s in range(B):
        ids = [int(b["hist_i"][s][k]) for k in range(min(int(b["sl"][s]), Ls))]
        ids += [int(np.asarray(b["hist_i_new"]).reshape(B, -1)[s][k]) for k in range(min(int(b["sl_new"][s]), Sn))]
        ids.append(int(b["i"][s]))
        for i in ids:
            rows["item"].setdefault(i, []).append(n)
            if cseg:
                rows["cate"].setdefault(int(item_cate[i]), []).append(n)
            n += 1
        rows["user"].setdefault(int(b["u"][s]), []).append(s)
        rows["cate"].setdefault(int(b["u_cate"][s]), []).append(s)
    return rows, n


@pytest.mark.parametrize("cseg", [False, True])
def test_tables_against_brute_force(cseg):
    for cfg, b, cat in _batches():
        U, I, C, Ls = cfg["user_count"], cfg["item_count"], cfg["cate_count"], cfg["Ls"]
        ref = R.build(b, U, I, C, Ls, cat, cseg=cseg)
        rows, n_item_uses = _brute(b, Ls, cat, cseg)
        B = len(b["u"])
        totals = dict(item=n_item_uses, user=B, cate=B + (n_item_uses if cseg else 0))
        for name, n in (("item", I), ("user", U), ("cate", C)):
            t, br = ref[name], rows[name]
            assert t["cnt"].tolist() == [len(br.get(r, [])) for r in range(n)]
            # the segments tile [0, total) without gaps, in row order
            pos = 0
            for r in range(n):
                assert t["off"][r] == pos
                pos += len(br.get(r, []))
            assert t["off"][n] == pos == totals[name]
            # records: the used rows ascending, their segments, counts that add up to the uses
            assert t["n_uniq"] == len(br) == len(t["rec"])
            assert t["rec"][:, 0].tolist() == sorted(br)
            assert (np.diff(t["rec"][:, 0]) > 0).all()
            assert t["rec"][:, 2].sum() == totals[name]
            for row, first, count, zero in t["rec"].tolist():
                assert (first, count, zero) == (t["off"][row], len(br[row]), 0)
        for hot in (0, 3, 48):
            slots = R.hot_slots(ref["item"]["rec"], hot)
            assert slots == {k for k, row in enumerate(sorted(rows["item"])) if len(rows["item"][row]) > hot}
        assert ref["lists"] == [{s for s in range(B) if b["u_cate"][s] == c} for c in range(C)]


def _brute_rank(b, Ls, Sn, by_window):
    keys = []
    for s in range(len(b["sl"])):
        w, n = max(min(int(b["sl"][s]), Ls), 0), max(min(int(b["sl_new"][s]), Sn), 0)
        if by_window > 0:
            keys.append(min(w, 191))
        elif min(n, 15) >= 2:
            keys.append(11 * min(n, 15) + min(w, 10))
        else:
            keys.append(10 - min(w, 10))
    order = sorted(range(len(keys)), key=lambda s: (-keys[s], s))     # descending by key, ties in sample order
    return keys, order


@pytest.mark.parametrize("by_window", [1, 0, -1])
@pytest.mark.parametrize("B", [17, 32, 33, 250, 600])
def test_ranking_invariants(B, by_window):
    Ls, Sn = (33, 2) if by_window > 0 else (10, 5)
    cfg = make_config(Ls=Ls)
    for mix in ("random", "light", "heavy", "few"):
        b, _ = random_batch(cfg, B=B, Sn=Sn, seed=B + len(mix))
        if mix == "light":
            b["sl_new"] = np.minimum(b["sl_new"], 1)
        elif mix == "heavy":
            b["sl_new"] = np.maximum(b["sl_new"], 2)
        elif mix == "few":               # a heavy count that is no multiple of G
            b["sl_new"] = np.where(np.arange(B) % 7 == 3, 3, 1)
        G = (B + 15) // 16
        perm = R.ranking(b["sl"], b["sl_new"], Ls, Sn, by_window)
        keys, order = _brute_rank(b, Ls, Sn, by_window)
        assert R.rank_keys(b["sl"], b["sl_new"], Ls, Sn, by_window).tolist() == keys
        # every sample exactly once, 16 G - B pads, at most 16 entries per group (by construction of the shape)
        assert perm.shape == (16 * G,)
        assert sorted(perm[perm < B].tolist()) == list(range(B))
        assert (perm == B).sum() == 16 * G - B
        grid = perm.reshape(G, 16)
        rank_of = np.empty(B + 1, np.int64)
        rank_of[order] = np.arange(B)
        rank_of[B] = B       # (pads rank behind everything)
        n_heavy = 16 * G if by_window > 0 else sum(k > 10 for k in keys)
        H = min(16, -(-n_heavy // G))
        if mix == "light" and by_window <= 0:
            assert H == 0
        if mix == "heavy" and by_window <= 0:
            assert H == min(16, -(-B // G)) and (H == 16 or B <= 15 * G)     # (every round once B > 15 G)
        if mix == "few" and by_window <= 0:
            assert 0 < H < 16
        # round j < H gives every group one sample of the j-th stretch of G ranks (by_window: the j-th sixteenth)
        for j in range(H):
            got = np.minimum(rank_of[grid[:, j]], 16 * G)
            real = grid[:, j] < B
            assert ((got[real] >= j * G) & (got[real] < (j + 1) * G)).all()
            assert real.sum() == max(0, min(B, (j + 1) * G) - j * G)
            # snake: forwards on even rounds, backwards on odd ones; groups numbered backwards when by_window == 0
            seq = grid[:, j][::-1] if (j & 1) else grid[:, j]
            if by_window == 0:
                seq = seq[::-1]
            r = rank_of[seq[seq < B]]
            assert (np.diff(r) > 0).all()
        # the tail: contiguous runs of 16 - H ranks per group, in rank order
        if H < 16:
            tail = grid[:, H:] if by_window != 0 else grid[::-1, H:]
            flat = tail.reshape(-1)
            nt = B - min(B, H * G)
            assert (flat[:nt] < B).all() and (flat[nt:] == B).all()
            assert rank_of[flat[:nt]].tolist() == list(range(H * G, B))


def test_ranking_is_stable():
    """equal keys keep the batch's order: with one key for everybody the ranking is the identity"""
    B, Ls = 40, 33
    perm = R.ranking(np.full(B, 7), np.zeros(B, np.int64), Ls, 0, 1)
    G = 3
    back = np.full(16 * G, B)
    for r in range(16 * G):
        j, idx = divmod(r, G)
        back[(G - 1 - idx if j & 1 else idx) * 16 + j] = r if r < B else B
    assert perm.tolist() == back.tolist()


def test_cases_take_the_forms_they_were_written_for():
    """every case of the GPU test (tests/index_cases.py) against tlsan_index_plan_of, on the host: a changed threshold shows
    here as the case that no longer exercises its form -- and the reference builds every case's batch"""
    import ctypes as C
    from tests.index_cases import AP_HOT, AP_HOT_CAP, CASES, PLAN_FIELDS
    from tests.test_abi_cpu import _lib
    L, lib = _lib()
    seen = {f: set() for f in PLAN_FIELDS}
    for case in CASES:
        cfg = make_config(**case.cfg)
        dims = L.Dims(cfg["user_count"], cfg["item_count"], cfg["cate_count"], cfg["hidden_units"], cfg["itemid_embedding_size"],
                      cfg["cateid_embedding_size"], cfg["num_heads"], cfg["Ls"])
        plan, lay = L.IndexPlan(), L.IndexLayout()
        assert lib.tlsan_index_plan_of(C.byref(dims), case.B, case.Sn, case.flags, C.byref(plan)) == 0, case.name
        assert {f: getattr(plan, f) for f in PLAN_FIELDS} == case.plan, case.name
        for f in PLAN_FIELDS:
            seen[f].add(case.plan[f])
        assert lib.tlsan_index_layout_of(C.byref(dims), 2, C.byref(lay)) == 0
        assert (lay.ap_hot, lay.ap_hot_cap) == (AP_HOT, AP_HOT_CAP)
        assert 0 < lay.cnt_item < lay.flag_user < lib.tlsan_state_bytes(C.byref(dims))
        b, cat = case.batch(cfg)
        ref = R.build(b, cfg["user_count"], cfg["item_count"], cfg["cate_count"], cfg["Ls"], cat, cseg=bool(plan.cseg),
                      rank=bool(plan.rank), by_window=plan.by_window, ap_hot=AP_HOT)
        assert ref["user"]["off"][-1] == case.B
        if "hot" in case.name:
            want = int(case.name.split("-")[2]) if case.name.split("-")[3:4] == ["rows"] else 1
            assert len(ref["hot"]) == want, case.name
    assert all(len(v) >= 2 for v in seen.values()), seen      # every form is taken and not taken somewhere
    assert seen["sparse"] == {0, 4, 5} and seen["by_window"] == {0, 1}

"""Similar-items lists without a GPU: the ABI's additions, the argument checks of tlsan_item_vectors /
tlsan_similar_workspace_bytes / tlsan_similar_topk (refused before any launch), the driver's flags and the reference's
ordering rule (tests/similar_ref.py) on hand-made cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import similar_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_item_vectors", "tlsan_similar_workspace_bytes", "tlsan_similar_topk")


def test_header_and_exports():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, hdr), name
        assert name in L.EXPORTS
        assert hasattr(L.load(), name)
    for name, val in (("TLSAN_SIM_DOT", L.SIM_DOT), ("TLSAN_SIM_COSINE", L.SIM_COSINE)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m is not None and int(m.group(1)) == val, name
    assert (L.SIM_DOT, L.SIM_COSINE) == (0, 1)
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)
    assert L.ABI_VERSION == 15 and L.load().tlsan_abi_version() == 15


def test_arguments_are_refused_without_a_launch():
    from tlsan_amd import _lib as L
    lib = L.load()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    bad_dims = L.Dims(100, 200, 10, 128, 64, 32, 8, 10)       # d_item + d_cate != d
    fake = 0x1000                       # never dereferenced: every call below is refused by the argument checks
    p = L.Params(*([fake] * 8))
    hole = L.Params(*([fake] * 8))
    hole.item_cate = None
    err = lambda: lib.tlsan_last_error()

    def vectors(d=dims, pp=p, ids=fake, Q=4, mul=1, add=0, vec=fake, inv=fake):
        return lib.tlsan_item_vectors(C.byref(d) if d else None, C.byref(pp) if pp else None, ids, Q, mul, add, vec, inv, None)

    for kw in (dict(ids=None), dict(vec=None), dict(Q=0), dict(Q=-3), dict(d=None), dict(d=bad_dims), dict(pp=None),
               dict(pp=hole), dict(mul=0), dict(add=-1)):
        assert vectors(**kw) == -1, kw
        assert b"tlsan_item_vectors" in err(), (kw, err())

    ws_need = lib.tlsan_similar_workspace_bytes(C.byref(dims), 4, 16)
    assert ws_need >= 200 * 128 * 4 + 200 * 4         # the dense item matrix and the inverse norms
    for d, Q, K in ((bad_dims, 4, 16), (None, 4, 16), (dims, 0, 16), (dims, 4, 0), (dims, 4, 257)):
        assert lib.tlsan_similar_workspace_bytes(C.byref(d) if d else None, Q, K) == 0
        assert b"tlsan_similar_workspace_bytes" in err(), err()

    def topk(d=dims, pp=p, qvec=fake, qinv=fake, qids=fake, Q=4, K=16, metric=L.SIM_COSINE, off=None, xid=None, mul=1, add=0,
             ids=fake, scores=fake, ws=fake, ws_bytes=1 << 40):
        return lib.tlsan_similar_topk(C.byref(d) if d else None, C.byref(pp) if pp else None, qvec, qinv, qids, Q, K, metric,
                                      off, xid, mul, add, ids, scores, ws, C.c_size_t(ws_bytes), None)

    for kw in (dict(qvec=None), dict(qinv=None), dict(qids=None), dict(ids=None), dict(scores=None), dict(Q=0), dict(K=0),
               dict(K=257), dict(K=-1), dict(metric=2), dict(metric=-1), dict(d=None), dict(d=bad_dims), dict(pp=None),
               dict(pp=hole), dict(off=fake), dict(xid=fake), dict(mul=0), dict(add=-1)):
        assert topk(**kw) == -1, kw
        assert b"tlsan_similar_topk" in err(), (kw, err())
    for kw in (dict(ws=None), dict(ws_bytes=ws_need - 1), dict(ws_bytes=0), dict(metric=L.SIM_DOT, qinv=None, ws_bytes=0)):
        assert topk(**kw) == -2, kw        # (the last: a NULL qinv is fine for dot, the check moves on to the workspace)
        assert b"tlsan_similar_topk" in err(), (kw, err())
    unsupported = L.Dims(100, 200, 10, 96, 48, 48, 8, 10)     # a (d, heads) pair this build does not have
    assert topk(d=unsupported) == -4 and b"tlsan_similar_topk" in err()


def test_driver_parses_the_flags():
    from tlsan_amd import train as T
    args = T.parse(["--dataset", "x.npz"])
    assert args.similar_k == 0 and args.similar_metric == "cosine"
    args = T.parse(["--dataset", "x.npz", "--similar_k", "7", "--similar_metric", "dot"])
    assert args.similar_k == 7 and args.similar_metric == "dot"
    with pytest.raises(SystemExit):
        T.parse(["--dataset", "x.npz", "--similar_metric", "l2"])
    assert T.similar_path("m", 7) == os.path.join("m", "similar-7.npz")


def test_reference_order():
    nan = float("nan")
    s = np.array([0.5, 2.0, -0.0, 2.0, nan, 0.0, -1.0, nan, 0.5])
    ok = np.ones(9, bool)
    assert ref.order(s, ok).tolist() == [1, 3, 0, 8, 2, 5, 6, 4, 7]     # ties by id; +0 == -0; NaN last, by id
    ok[3] = False
    assert ref.order(s, ok).tolist() == [1, 0, 8, 2, 5, 6, 4, 7]
    ids, sc = ref.topk(s[None], ok[None], 10)
    assert ids[0].tolist() == [1, 0, 8, 2, 5, 6, 4, 7, -1, -1]
    assert sc[0, 8] == -np.inf and sc[0, 9] == -np.inf and np.isnan(sc[0, 6])
    assert sc[0, 3] == 0 and not np.signbit(sc[0, 3])                    # a zero score comes back as +0.0
    assert ref.order(np.array([-np.inf, np.inf, nan]), np.ones(3, bool)).tolist() == [1, 0, 2]


def test_reference_scores_and_eligibility():
    w = np.array([[1.0, 0.0], [2.0, 0.0], [0.0, 0.0], [0.0, 3.0], [-1.0, 0.0]])
    q = [0, 2]
    dot = ref.scores(w, q, "dot", P=0.5)
    assert dot[0].tolist() == [0.25, 0.5, 0.0, 0.0, -0.25] and not dot[1].any()
    cos = ref.scores(w, q, "cosine", P=0.5)
    assert cos[0].tolist() == [1.0, 1.0, 0.0, 0.0, -1.0] and not cos[1].any()       # a zero row: inv = 0
    ok = ref.eligible(5, q, [[1, 1, 77, -4], []])
    assert ok.tolist() == [[False, False, True, True, True], [True, True, False, True, True]]
    ids, sc = ref.topk(cos, ok, 4)
    assert ids.tolist() == [[2, 3, 4, -1], [0, 1, 3, 4]]
    tol = ref.tolerance(w, q, "cosine")
    ref.check_lists(ids.astype(np.int32), sc.astype(np.float32), cos, ok, tol)
    swapped = ids.copy()
    swapped[1, :2] = [1, 0]
    with pytest.raises(AssertionError):
        ref.check_lists(swapped.astype(np.int32), sc.astype(np.float32), cos, ok, tol)
    with pytest.raises(AssertionError):                                              # the query in its own list
        ref.check_lists(np.array([[0, 2, 3, 4]], np.int32), np.array([[1, 0, 0, -1]], np.float32), cos[:1], ok[:1], tol[:1])

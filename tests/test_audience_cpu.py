"""Audience lists without a GPU: the numpy reference against a python-loop brute force, the torch item -> rows
transposition on CPU tensors against its brute force, the workspace size of tlsan_dense_topk, every refusal of the raw
call on fake pointers (no launch), the ValueErrors of the python layer that need no device, and the driver's parse errors."""
import os
import re

import numpy as np
import pytest

from tests import audience_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000            # never dereferenced: every call below is refused before any launch
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def test_reference_equals_the_brute_force_on_small_cases_with_ties():
    rng = np.random.RandomState(3)
    for case in range(40):
        Q, N, k = rng.randint(1, 5), rng.randint(1, 14), rng.randint(1, 17)
        s = rng.randint(-2, 3, (Q, N)).astype(np.float32)           # few distinct values: ties everywhere
        s[rng.rand(Q, N) < 0.15] = -0.0
        s[rng.rand(Q, N) < 0.1] = np.nan
        s[rng.rand(Q, N) < 0.05] = np.inf
        s[rng.rand(Q, N) < 0.05] = -np.inf
        id_add = int(rng.choice([0, 7, 1000]))
        excl = None if case % 3 == 0 else [rng.randint(id_add - 2, id_add + N + 2, rng.randint(0, N + 2)) for _ in range(Q)]
        got, want = ref.expected(s, k, excl, id_add), ref.brute_force(s, k, excl, id_add)
        assert np.array_equal(got[0], want[0]), case
        assert np.array_equal(np.isnan(got[1]), np.isnan(want[1])), case
        fin = ~np.isnan(got[1])
        assert np.array_equal(got[1][fin].view(np.int32), want[1][fin].view(np.int32)), case   # (bits: a zero is +0.0)
        assert got[0].dtype == np.int32 and got[1].dtype == np.float32


def test_reference_details():
    s = np.array([[1.0, np.nan, 1.0, -0.0, 0.0, np.inf, -np.inf]], np.float32)
    rows, sc = ref.expected(s, 9)
    assert rows[0].tolist() == [5, 0, 2, 3, 4, 6, 1, -1, -1]          # +inf, the ties by row, the zeros equal, -inf, NaN, padding
    assert not np.signbit(sc[0, 3]) and not np.signbit(sc[0, 4]) and np.isnan(sc[0, 6]) and (sc[0, 7:] == -np.inf).all()
    rows, _ = ref.expected(s, 3, exclude=[[105, 100, 3, 999]], id_add=100)   # (3 and 999 are outside [100, 107))
    assert rows[0].tolist() == [102, 103, 104]


def _csr(lists):
    off = np.cumsum([0] + [len(x) for x in lists])
    return off, np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])


def test_transposition_equals_the_brute_force_on_cpu_tensors():
    import torch
    from tlsan_amd.model import seen_rows_csr
    rng = np.random.RandomState(5)
    for case in range(25):
        n_users, n_items, N = rng.randint(1, 12), rng.randint(2, 20), rng.randint(1, 40)
        seen = [np.sort(rng.choice(n_items, rng.randint(0, min(n_items, 6)), replace=False)) for _ in range(n_users)]
        if case % 4 == 0:
            seen[0] = np.array([1, 1, 1])                             # a list that repeats an item: the row counts once
        off, ids = _csr(seen)
        # users with several rows, users with none, and user ids outside the CSR (nothing seen)
        user = rng.randint(-1, n_users + 2, N)
        user[rng.rand(N) < 0.3] = rng.randint(0, n_users)
        items = rng.randint(0, n_items + 3, rng.randint(1, 9))       # items nobody has seen, ids past every list
        items[-1] = items[0]                                          # a repeated query item
        row0 = int(rng.choice([0, 17]))
        want = ref.seen_rows(off, ids, user, items, row0)
        goff, grows = seen_rows_csr(torch.as_tensor(off), torch.as_tensor(ids), torch.as_tensor(user.astype(np.int32)),
                                    torch.as_tensor(items), row0)
        assert goff.dtype == torch.int32 and grows.dtype == torch.int32 and goff.shape == (len(items) + 1,)
        goff, grows = goff.numpy(), grows.numpy()
        assert goff[0] == 0 and len(grows) >= max(goff[-1], 1)
        for q in range(len(items)):
            assert grows[goff[q]:goff[q + 1]].tolist() == want[q], (case, q)


def test_transposition_edge_cases():
    import torch
    from tlsan_amd.model import seen_rows_csr
    off, ids = torch.tensor([0, 0, 0]), torch.zeros(0, dtype=torch.int64)           # nobody has seen anything
    goff, grows = seen_rows_csr(off, ids, torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([0, 5]))
    assert goff.tolist() == [0, 0, 0] and grows.numel() >= 1
    off, ids = torch.tensor([0, 2]), torch.tensor([4, 9])                            # one user, every row theirs
    goff, grows = seen_rows_csr(off, ids, torch.zeros(5, dtype=torch.int32), torch.tensor([9, 9, 4, 3]), row0=100)
    assert goff.tolist() == [0, 5, 10, 15, 15] and grows[:15].tolist() == [100, 101, 102, 103, 104] * 3


def test_workspace_bytes_positive_and_monotone():
    from tlsan_amd import _lib as L
    lib = L.load()
    f = lib.tlsan_dense_topk_workspace_bytes
    assert f(1, 1, 1) > 0
    Qs = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 100, 256, 257, 1000, 4096, 4097, 32768, 32769, 100000, 1 << 24]
    Ns = [1, 16, 17, 256, 257, 600, 1024, 1025, 65536, 200000, 10 ** 7, 1 << 30]
    Ks = [1, 10, 16, 17, 64, 65, 100, 256]
    for K in Ks:
        for N in Ns:
            v = [f(Q, N, K) for Q in Qs]
            assert all(x > 0 for x in v) and all(a <= b for a, b in zip(v, v[1:])), ("Q", N, K, v)
        for Q in Qs:
            v = [f(Q, N, K) for N in Ns]
            assert all(a <= b for a, b in zip(v, v[1:])), ("N", Q, K, v)
    for Q in Qs:
        for N in Ns:
            v = [f(Q, N, K) for K in Ks]
            assert all(a <= b for a, b in zip(v, v[1:])), ("K", Q, N, v)
    # the room covers the slices' lists: Q * slices * K ids and as many scores (eval_slices: ceil(2048 / tiles), as many as there is work for)
    for Q, N, K in ((1, 600, 10), (17, 10 ** 7, 100), (4096, 200000, 10), (40, 257, 64)):
        ut, n = (Q + 15) // 16, ((N + 63) // 64 + 3) // 4
        nsl = max(1, min(n, (2048 + ut - 1) // ut))
        assert f(Q, N, K) >= 2 * 4 * Q * nsl * K
    for bad in ((0, 10, 1), (-1, 10, 1), ((1 << 24) + 1, 10, 1), (4, 0, 1), (4, -5, 1), (4, (1 << 30) + 1, 1), (4, 10, 0),
                (4, 10, 257), (4, 10, -1)):
        assert f(*bad) == 0 and lib.tlsan_last_error().startswith(b"tlsan_dense_topk_workspace_bytes"), bad


def test_every_refusal_of_the_raw_call_names_its_entry_point():
    from tlsan_amd import _lib as L, build
    lib = L.load()
    with open(os.path.join(ROOT, "include", "tlsan.h")) as fh:
        header = fh.read()
    for name in ("tlsan_dense_topk_workspace_bytes", "tlsan_dense_topk"):
        assert name in L.EXPORTS and hasattr(lib, name) and re.search(r"\b%s\(" % name, header), name
    assert "tlsan_dense.hip" in build.SOURCES and L.ABI_VERSION == 15 and lib.tlsan_abi_version() == 15
    need = lib.tlsan_dense_topk_workspace_bytes(40, 600, 10)
    good = dict(q=FAKE, Q=40, d=128, x=FAKE, N=600, q_scale=None, q_bias=None, excl_off=None, excl_ids=None, id_add=0, K=10,
                ids=FAKE, scores=FAKE, ws=FAKE, ws_bytes=need)
    order = list(good)
    cases = [(dict(q=None), BADARG), (dict(x=None), BADARG), (dict(ids=None), BADARG), (dict(scores=None), BADARG),
             (dict(ws=None), WORKSPACE), (dict(excl_off=FAKE), BADARG), (dict(excl_ids=FAKE), BADARG),
             (dict(Q=0), BADARG), (dict(Q=-3), BADARG), (dict(N=0), BADARG), (dict(N=-1), BADARG),
             (dict(N=(1 << 31) - 1), BADARG), (dict(N=600, id_add=(1 << 31) - 600 + 1), BADARG),
             (dict(N=1 << 30, id_add=(1 << 30) + 1, ws_bytes=1 << 62), BADARG),
             (dict(d=96), UNSUPPORTED), (dict(d=0), UNSUPPORTED), (dict(d=512), UNSUPPORTED),
             (dict(K=0), BADARG), (dict(K=257), BADARG), (dict(K=-1), BADARG), (dict(id_add=-1), BADARG),
             (dict(ws_bytes=need - 1), WORKSPACE), (dict(ws_bytes=0), WORKSPACE)]
    for change, code in cases:
        kw = dict(good, **change)
        rc = lib.tlsan_dense_topk(*[kw[k] for k in order], None)
        msg = lib.tlsan_last_error()
        assert rc == code and msg.startswith(b"tlsan_dense_topk:"), (change, rc, msg)


def test_value_errors_that_need_no_gpu():
    import torch
    from tlsan_amd.model import UserVectors, audience_exclusion, audience_queries, batch_list, check_user_vectors, kept_rows
    assert audience_queries([3, 3, 0], 10, 40, "cpu").tolist() == [3, 3, 0]         # repeats are allowed
    for items, k in (([3], 0), ([3], 257), ([3], 2.5), ([3], True), ([40], 5), ([-1], 5), ([], 5), ([[1, 2]], 5), ([1.5], 5)):
        with pytest.raises(ValueError):
            audience_queries(items, k, 40, "cpu")
    owner, other = object(), object()
    uv = UserVectors(torch.zeros(5, 64), torch.arange(5), owner, 7)
    assert len(uv) == 5 and uv.row0 == 0 and uv.n_total == 5 and uv.user.dtype == torch.int32
    check_user_vectors(uv, owner, 7, 64, "cpu")
    for args in ((uv, other, 7, 64, "cpu"), (uv, owner, 8, 64, "cpu"), (uv, owner, 7, 128, "cpu"), (uv, owner, 7, 64, "cuda:0"),
                 (torch.zeros(5, 64), owner, 7, 64, "cpu"), (None, owner, 7, 64, "cpu")):
        with pytest.raises(ValueError):
            check_user_vectors(*args)
    with pytest.raises(ValueError):
        check_user_vectors(UserVectors(torch.zeros(5, 64, dtype=torch.float64), torch.arange(5), owner, 7), owner, 7, 64, "cpu")
    # users_of: rows -> user ids, -1 stays -1
    uv = UserVectors(torch.zeros(3, 64), torch.tensor([9, 4, 9]), owner, 0)
    assert uv.users_of(np.array([[2, 0, -1], [1, -1, -1]])).tolist() == [[9, 9, -1], [4, -1, -1]]
    # exclusion forms
    q = torch.tensor([1, 2], dtype=torch.int32)
    assert audience_exclusion(None, q, uv) == (None, None)
    off, ids = audience_exclusion([[2, 0, 2, 77, -4], []], q, uv)                    # sorted, repeats and foreign rows dropped
    w = int(off[1])
    assert off.tolist() == [0, w, 2 * w] and ids[:2].tolist() == [0, 2] and (ids[2:] == np.iinfo(np.int32).max).all()
    for bad in ("history", [[1]], [[1], [2], [3]]):
        with pytest.raises(ValueError):
            audience_exclusion(bad, q, uv)
    one = (np.zeros(3), np.zeros(3))
    for got, n in ((batch_list(one), 1), (batch_list([one, one]), 2), (batch_list(iter([one])), 1), (batch_list((one, one)), 2)):
        assert len(got) == n and all(b is one for b in got)
    assert kept_rows(None, 2) == [None, None] and kept_rows([3, 0], 2) == [3, 0] and kept_rows(4, 1) == [4]
    for real, n in (([1], 2), ([1, -1], 2)):
        with pytest.raises(ValueError):
            kept_rows(real, n)


def test_driver_parse_errors(capsys):
    from tlsan_amd.train import parse
    a = parse(["--audience_k", "5", "--audience_items", "3,7,12", "--audience_exclude", "seen"])
    assert (a.audience_k, a.audience_items, a.audience_exclude) == (5, [3, 7, 12], "seen")
    a = parse([])
    assert (a.audience_k, a.audience_items, a.audience_exclude) == (0, [], "none")
    for argv, word in ((["--audience_k", "5"], "--audience_items"),                  # required with --audience_k
                       (["--audience_items", "3,7"], "--audience_k"),
                       (["--audience_exclude", "seen"], "--audience_k"),
                       (["--audience_k", "5", "--audience_items", "3,x"], "--audience_items"),
                       (["--audience_k", "5", "--audience_items", "3,-7"], "non-negative"),
                       (["--audience_k", "257", "--audience_items", "3"], "--audience_k"),
                       (["--audience_k", "-1", "--audience_items", "3"], "--audience_k"),
                       (["--audience_k", "5", "--audience_items", "3", "--audience_exclude", "history"], "invalid choice")):
        with pytest.raises(SystemExit):
            parse(argv)
        assert word in capsys.readouterr().err, argv

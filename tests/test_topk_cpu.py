"""Top-K recommendation over all items, the parts that need no GPU: the C ABI declares and exports the three entry
points, the workspace query refuses bad K / dims, NULL arguments are refused before the device is touched, and the
driver's flags and output naming."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tlsan_topk_workspace_bytes", "tlsan_eval_topk", "tlsan_topk_merge")


def _lib():
    from tlsan_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from tlsan_amd.build import build
        build()
    return L, L.load()


def test_topk_symbols_declared_and_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    declared = set(re.findall(r"\b(tlsan_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in L.EXPORTS, name
        assert hasattr(lib, name), name
    assert L.TOPK_MAX == 256


def test_topk_workspace_bytes():
    L, lib = _lib()
    for d in (64, 128, 256):
        dims = L.Dims(100, 22048, 10, d, d // 2, d // 2, 8, 10)
        for k in (1, 10, 50, 256):
            assert lib.tlsan_topk_workspace_bytes(C.byref(dims), 4096, k) > 0, (d, k)
        for k in (0, -1, 257):
            assert lib.tlsan_topk_workspace_bytes(C.byref(dims), 4096, k) == 0, (d, k)
            assert b"K must be in 1..256" in lib.tlsan_last_error()
        assert lib.tlsan_topk_workspace_bytes(C.byref(dims), 0, 10) == 0
    # the slices' lists grow with K; a table too large for the dense item matrix needs none of it
    dims = L.Dims(100, 22048, 10, 128, 64, 64, 8, 10)
    assert lib.tlsan_topk_workspace_bytes(C.byref(dims), 4096, 256) > lib.tlsan_topk_workspace_bytes(C.byref(dims), 4096, 10)
    big = L.Dims(100, 300000, 10, 256, 128, 128, 8, 10)
    assert lib.tlsan_topk_workspace_bytes(C.byref(big), 4096, 10) < 300000 * 256 * 4
    bad = L.Dims(100, 200, 10, 96, 48, 48, 8, 10)
    assert lib.tlsan_topk_workspace_bytes(C.byref(bad), 16, 10) == 0
    assert b"unsupported" in lib.tlsan_last_error()
    assert lib.tlsan_topk_workspace_bytes(None, 16, 10) == 0


def test_topk_null_arguments_are_rejected_not_crashed():
    L, lib = _lib()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    assert lib.tlsan_eval_topk(C.byref(dims), None, None, 16, 10, None, None, 1, 0, None, None, None, 0, None) == -1
    assert lib.tlsan_eval_topk(None, None, None, 16, 10, None, None, 1, 0, None, None, None, 0, None) == -1
    assert lib.tlsan_topk_merge(None, None, 16, 2, 10, None, None, None) == -1
    # non-NULL but fake pointers: the argument checks refuse before any launch
    fake = C.c_void_p(0x1000)
    assert lib.tlsan_topk_merge(fake, fake, 16, 2, 0, fake, fake, None) == -1
    assert lib.tlsan_topk_merge(fake, fake, 16, 2, 257, fake, fake, None) == -1
    assert lib.tlsan_topk_merge(fake, fake, 0, 2, 10, fake, fake, None) == -1
    assert lib.tlsan_topk_merge(fake, fake, 16, 0, 10, fake, fake, None) == -1
    p = L.Params(*([fake.value] * 8))
    for k in (0, 257):
        assert lib.tlsan_eval_topk(C.byref(dims), C.byref(p), fake, 16, k, None, None, 1, 0, fake, fake, fake, 1 << 30,
                                   None) == -1
        assert b"K must be in 1..256" in lib.tlsan_last_error()
    # the exclusion CSR comes as a pair; the global ids must stay int32
    assert lib.tlsan_eval_topk(C.byref(dims), C.byref(p), fake, 16, 10, fake, None, 1, 0, fake, fake, fake, 1 << 30,
                               None) == -1
    assert lib.tlsan_eval_topk(C.byref(dims), C.byref(p), fake, 16, 10, None, None, 0, 0, fake, fake, fake, 1 << 30,
                               None) == -1
    assert lib.tlsan_eval_topk(C.byref(dims), C.byref(p), fake, 16, 10, None, None, 1 << 24, 0, fake, fake, fake,
                               1 << 30, None) == -1
    assert lib.tlsan_eval_topk(C.byref(dims), C.byref(p), fake, 16, 10, None, None, 1, 0, fake, fake, None, 0, None) == -2
    assert lib.tlsan_eval_topk(C.byref(dims), C.byref(p), fake, 16, 10, None, None, 1, 0, fake, fake, fake, 16,
                               None) == -2   # workspace too small
    assert b"workspace too small" in lib.tlsan_last_error()


def test_driver_recommend_flags(tmp_path):
    import numpy as np
    from tlsan_amd.train import parse, recommend_path, write_recommendations
    a = parse(["--dataset", "x.npz"])
    assert a.recommend_k == 0 and a.recommend_exclude == "history"       # off by default
    a = parse(["--dataset", "x.npz", "--recommend_k", "20", "--recommend_exclude", "none"])
    assert a.recommend_k == 20 and a.recommend_exclude == "none"
    with pytest.raises(SystemExit):
        parse(["--recommend_exclude", "all"])
    assert recommend_path("save_path", 20) == os.path.join("save_path", "recommend_top20.npz")
    path = write_recommendations(str(tmp_path), 3, np.arange(2), np.array([[5, 1, -1], [2, 0, 7]]),
                                 np.array([[1.0, 0.5, -np.inf], [2.0, 1.0, 0.0]]))
    z = np.load(path)
    assert path == recommend_path(str(tmp_path), 3)
    assert sorted(z.files) == ["ids", "scores", "user"]
    assert z["ids"].dtype == np.int32 and z["scores"].dtype == np.float32 and z["ids"].shape == (2, 3)

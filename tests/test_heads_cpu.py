"""Host-side checks of the (hidden_units, num_heads) pairs the library is built for: the six supported pairs size their
state and workspace, every other pair is refused as unsupported (no GPU needed)."""
import ctypes as C
import os

import pytest

SUPPORTED = [(64, 8), (128, 8), (256, 8), (64, 4), (128, 16), (128, 4)]
# dh = 4 (4 heads per 16-channel block), dh = 64 (4 blocks per column), 64/2 (2 columns per sample: 8 lanes for 13 use
# slots), 256/16 and 256/32 (16 columns per sample: 16-wavefront workgroups), d = 96
UNSUPPORTED = [(64, 16), (128, 32), (128, 2), (256, 4), (64, 2), (256, 16), (256, 32), (96, 8), (96, 4)]


def _lib():
    from tlsan_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from tlsan_amd.build import build
        build()
    return L, L.load()


@pytest.mark.parametrize("d,h", SUPPORTED)
@pytest.mark.parametrize("Ls", [10, 90])
def test_supported_pairs_have_sizes(d, h, Ls):
    L, lib = _lib()
    dh = d // h
    dims = L.Dims(100, 200, 10, d, d // 2, d // 2, h, Ls)
    lay = L.DenseLayout()
    assert lib.tlsan_dense_layout_of(C.byref(dims), C.byref(lay)) == 0
    assert lay.n_dense == 4 * dh * dh + 4 * dh + d * d + d + 1
    assert lib.tlsan_state_bytes(C.byref(dims)) > 0
    w1 = lib.tlsan_workspace_bytes(C.byref(dims), 32, 4)
    w2 = lib.tlsan_workspace_bytes(C.byref(dims), 4096, 18)
    assert 0 < w1 < w2


@pytest.mark.parametrize("d,h", UNSUPPORTED)
def test_other_pairs_are_unsupported(d, h):
    L, lib = _lib()
    dims = L.Dims(100, 200, 10, d, d // 2, d // 2, h, 10)
    assert lib.tlsan_state_bytes(C.byref(dims)) == 0
    assert b"unsupported" in lib.tlsan_last_error()
    assert lib.tlsan_workspace_bytes(C.byref(dims), 32, 4) == 0
    assert b"unsupported" in lib.tlsan_last_error()


def test_refusal_names_the_supported_set():
    L, lib = _lib()
    dims = L.Dims(100, 200, 10, 256, 128, 128, 16, 10)
    assert lib.tlsan_state_bytes(C.byref(dims)) == 0
    msg = lib.tlsan_last_error().decode()
    for d, h in SUPPORTED:
        assert "%d/%d" % (d, h) in msg

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


@pytest.mark.parametrize("d,h", SUPPORTED)
def test_dense_layout_table_covers_the_vector_once_and_round_trips(d, h):
    """tlsan_amd.model.dense_slices is the one statement of where each dense weight sits: its slices hold every
    DENSE_KEYS name once, lie inside the packed vector without overlap, leave nothing but the layout's alignment padding
    (n_dense less the weights' own sizes) uncovered, and unpack_dense(pack_dense(p)) gives p back bit for bit."""
    import numpy as np
    from tlsan_amd.model import DENSE_KEYS, Model, dense_slices, pack_dense, unpack_dense
    L, lib = _lib()
    dims = L.Dims(100, 200, 10, d, d // 2, d // 2, h, 10)
    lay = L.DenseLayout()
    assert lib.tlsan_dense_layout_of(C.byref(dims), C.byref(lay)) == 0
    table = dense_slices(lay, d, h)
    assert sorted(name for name, _, _ in table) == sorted(DENSE_KEYS)
    dh = d // h
    want = dict(dense_K=(d, d), dense_b=(d,), gamma=())
    for blk in ("fwa1", "fwa2"):
        want.update({blk + "_W1": (dh, dh), blk + "_b1": (dh,), blk + "_W2": (dh, dh), blk + "_b2": (dh,)})
    covered = np.zeros(lay.n_dense, np.int64)
    for name, off, shape in table:
        assert tuple(shape) == want[name], name
        n = int(np.prod(shape)) if shape else 1
        assert 0 <= off and off + n <= lay.n_dense, name
        covered[off:off + n] += 1
    assert covered.max() == 1                                   # no overlap
    weights = 4 * dh * dh + 4 * dh + d * d + d + 1
    assert int(covered.sum()) == weights and int((covered == 0).sum()) == lay.n_dense - weights
    # values no two of which share a bit pattern, -0.0 and a denormal among them
    rng = np.random.RandomState(d * 100 + h)
    p = {name: rng.standard_normal(shape).astype(np.float32) for name, shape in want.items()}
    p["dense_b"][:2] = np.float32(-0.0), np.float32(1e-41)
    flat = pack_dense(lay, d, h, p)
    assert flat.dtype == np.float32 and flat.shape == (lay.n_dense,)
    assert not flat[covered == 0].any()                         # the padding stays zero
    back = unpack_dense(lay, d, h, flat)
    assert sorted(back) == sorted(DENSE_KEYS)
    for name in DENSE_KEYS:
        assert back[name].shape == want[name] and back[name].dtype == np.float32, name
        assert back[name].tobytes() == p[name].tobytes(), name
    # the reference's initial values go through the same table (Model.init_params names every dense weight)
    cfg = dict(item_count=3, user_count=3, cate_count=2, itemid_embedding_size=d // 2, cateid_embedding_size=d // 2,
               hidden_units=d, num_heads=h, Ls=10)
    init = Model.init_params(cfg, seed=5)
    back = unpack_dense(lay, d, h, pack_dense(lay, d, h, init))
    for name in DENSE_KEYS:
        assert back[name].tobytes() == np.asarray(init[name], np.float32).tobytes(), name

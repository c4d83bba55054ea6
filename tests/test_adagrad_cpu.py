"""Lazy Adagrad / row-wise Adagrad without a GPU: the ABI's kinds, the optimizer table, the argument checks of
tlsan_train_step_opt (refused before any launch), the driver's switches, the one-slot checkpoint and the reference rule
(tests/adagrad_ref.py) against torch.optim.Adagrad."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from tests import adagrad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adagrad_kinds_in_header_and_lib():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    for name, val in (("TLSAN_OPT_ADAGRAD", L.OPT_ADAGRAD), ("TLSAN_OPT_ROWWISE_ADAGRAD", L.OPT_ROWWISE_ADAGRAD)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, hdr)
        assert m is not None, name
        assert int(m.group(1)) == val
    assert (L.OPT_ADAGRAD, L.OPT_ROWWISE_ADAGRAD) == (4, 5)
    assert re.search(r"#define\s+TLSAN_ABI_VERSION\s+15\b", hdr)


def test_optimizer_table():
    from tlsan_amd import _lib as L
    from tlsan_amd.model import LAZY_ADAGRAD_OPTIMIZERS, LAZY_OPTIMIZERS, OPTIMIZERS
    assert set(LAZY_OPTIMIZERS) == {"lazy_adam", "lazy_rmsprop", "lazy_adadelta"}
    assert set(LAZY_ADAGRAD_OPTIMIZERS) == set(ref.KINDS)
    assert OPTIMIZERS["lazy_adagrad"][0] == L.OPT_ADAGRAD | L.OPT_LAZY
    assert OPTIMIZERS["lazy_rowwise_adagrad"][0] == L.OPT_ROWWISE_ADAGRAD | L.OPT_LAZY


def test_adagrad_kinds_are_refused_without_a_launch():
    from tlsan_amd import _lib as L
    lib = L.load()
    dims = L.Dims(100, 200, 10, 128, 64, 64, 8, 10)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused by the argument checks
    state = C.c_void_p(0x100000)
    p = L.Params(*([fake.value] * 8))
    p.scale = lib.tlsan_state_scale(state)
    slot = L.Params(*([fake.value] * 6))
    b = L.Batch(16, 2, *([fake.value] * 10))
    ws_bytes = 1 << 40

    def call(kind, l2_mode, norm_mode=L.NORM_TF18, slots=True, params=p):
        hp = L.HParams(0.1, 1e-4, 5.0, norm_mode, l2_mode, 0, 0, 0.0, 0, 0)
        opt = L.Optimizer(kind, 1, 0.0, 0.0, 0.0, C.addressof(slot) if slots else None, None)   # (slot2 may be NULL)
        return lib.tlsan_train_step_opt(C.byref(dims), C.byref(params), C.byref(b), C.byref(hp), C.byref(opt), None,
                                        state, fake, C.c_size_t(ws_bytes), None)

    for kind in (L.OPT_ADAGRAD, L.OPT_ROWWISE_ADAGRAD):
        for l2 in (L.L2_DENSE, L.L2_LAZY):
            assert call(kind, l2) == -4                        # no dense sweep
            assert b"dense sweep" in lib.tlsan_last_error()
        lk = kind | L.OPT_LAZY
        assert call(lk, L.L2_DENSE) == -4                      # needs the lazy tail
        assert b"TLSAN_L2_LAZY" in lib.tlsan_last_error()
        assert call(lk, L.L2_LAZY, L.NORM_DEDUP) == -4         # the TF18 norm only
        assert call(lk, L.L2_DENSE, L.NORM_DEDUP) == -4
        assert call(lk, L.L2_LAZY, slots=False) == -1          # no slot tables
        assert b"slot1" in lib.tlsan_last_error()
        q = L.Params(*([fake.value] * 8))                      # the table scale must be the state's
        assert call(lk, L.L2_LAZY, params=q) == -1
    hole = L.Params(*([fake.value] * 6))                       # a NULL table in slot1
    hole.cate_emb = None
    hp = L.HParams(0.1, 1e-4, 5.0, L.NORM_TF18, L.L2_LAZY, 0, 0, 0.0, 0, 0)
    opt = L.Optimizer(L.OPT_ROWWISE_ADAGRAD | L.OPT_LAZY, 1, 0.0, 0.0, 0.0, C.addressof(hole), None)
    assert lib.tlsan_train_step_opt(C.byref(dims), C.byref(p), C.byref(b), C.byref(hp), C.byref(opt), None, state, fake,
                                    C.c_size_t(ws_bytes), None) == -1
    assert b"slot1" in lib.tlsan_last_error()
    assert call(L.OPT_LAZY | 7, L.L2_LAZY) == -1               # (still no kind 7)
    assert call(7, L.L2_DENSE) == -1


def test_driver_parses_the_adagrad_names():
    from tlsan_amd import train as T
    from tlsan_amd.model import OPTIMIZERS
    for name in ref.KINDS:
        args = T.parse(["--dataset", "x.npz", "--optimizer", name, "--learning_rate", "0.05"])
        assert args.optimizer == name and args.learning_rate == 0.05 and args.optimizer in OPTIMIZERS


_SHARDED_REFUSAL = r"""
import os, sys, tempfile
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from tests.helpers import make_config
from tlsan_amd.dist import ShardedModel
init = "file://" + os.path.join(tempfile.mkdtemp(), "pg")
dist.init_process_group("gloo", init_method=init, rank=0, world_size=1)
try:
    for name in ("lazy_adagrad", "lazy_rowwise_adagrad"):
        for l2_mode in ("dense", "lazy"):
            try:
                ShardedModel(make_config(optimizer=name), list(range(40)), device="cpu", l2_mode=l2_mode)
            except NotImplementedError as e:
                assert name in str(e), e
            else:
                raise SystemExit("%s was accepted" % name)
finally:
    dist.destroy_process_group()
print("refused")
"""


def test_sharded_model_refuses_the_adagrad_names():
    """ShardedModel refuses both names beside its optimizer check, ahead of any device work (a world-1 gloo group in a
    child process)."""
    r = subprocess.run([sys.executable, "-c", _SHARDED_REFUSAL, ROOT], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


def test_checkpoint_round_trips_one_row_shaped_slot_set(tmp_path):
    from tlsan_amd.model import DENSE_KEYS, TABLE_KEYS, read_checkpoint, write_checkpoint
    from tests.helpers import make_config, random_params
    cfg = make_config(U=9, I=7, C=3)
    p = {k: np.asarray(v, np.float32) for k, v in random_params(cfg, seed=3).items()}
    assert set(p) == set(TABLE_KEYS + DENSE_KEYS)
    slot = {k: np.asarray(v, np.float32) for k, v in ref.random_accumulators(p, "lazy_rowwise_adagrad", 4).items()}
    assert slot["item_emb"].shape == (7,) and slot["usert_emb"].shape == (9,) and slot["item_b"].shape == (7,)
    path = str(tmp_path / "TLSAN-5.npz")
    write_checkpoint(path, 5, 1, p, [slot])
    step, epoch, q, slots = read_checkpoint(path)
    assert (step, epoch) == (5, 1) and isinstance(slots, list) and len(slots) == 1
    for k in p:
        assert np.array_equal(q[k], p[k]) and np.array_equal(slots[0][k], slot[k]) and slots[0][k].shape == slot[k].shape, k
    write_checkpoint(path, 5, 1, p, [slot, slot])           # (two sets are still read as two)
    assert len(read_checkpoint(path)[3]) == 2
    assert read_checkpoint(path, want_slots=False)[3] is None


def test_elementwise_rule_is_torch_adagrad():
    import torch
    rng = np.random.RandomState(11)
    w = rng.uniform(-1, 1, (13, 7))
    t = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adagrad([t], lr=0.05, initial_accumulator_value=0.1, eps=0)
    acc = np.full(w.shape, 0.1)
    for _ in range(3):
        g = rng.uniform(-0.3, 0.3, w.shape)
        t.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        w, acc = ref.elementwise_rule(w, g, acc, 0.05)
        assert np.abs(t.detach().numpy() - w).max() < 1e-12
    assert np.abs(opt.state[t]["sum"].numpy() - acc).max() < 1e-12


def test_rowwise_rule_on_width_one_is_the_elementwise_rule():
    rng = np.random.RandomState(12)
    w, acc = rng.uniform(-1, 1, (17, 1)), rng.uniform(0.05, 0.5, 17)
    we, ae = w.copy(), acc.reshape(17, 1).copy()
    for _ in range(3):
        g = rng.uniform(-0.3, 0.3, (17, 1))
        w, acc = ref.rowwise_rule(w, g, acc, 0.05)
        we, ae = ref.elementwise_rule(we, g, ae, 0.05)
        assert np.array_equal(w, we) and np.array_equal(acc, ae[:, 0])
    wide_w, wide_acc = ref.rowwise_rule(np.ones((2, 4)), np.array([[1.0, 1, 1, 1], [2.0, 0, 0, 0]]), np.zeros(2), 1.0)
    assert np.array_equal(wide_acc, [1.0, 1.0]) and np.array_equal(wide_w, [[0.0, 0, 0, 0], [-1.0, 1, 1, 1]])

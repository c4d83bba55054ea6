"""Lazy Adam / RMSProp / Adadelta without a GPU: the ABI flag, the optimizer table, the argument checks of
tlsan_train_step_opt (refused before any launch) and the driver's switches."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from tlsan_amd import _lib as L
    return L, L.load()


def test_lazy_flag_in_header_and_lib():
    from tlsan_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    m = re.search(r"#define\s+TLSAN_OPT_LAZY\s+(0x[0-9a-fA-F]+|\d+)", hdr)
    assert m is not None
    assert int(m.group(1), 0) == L.OPT_LAZY
    assert L.OPT_LAZY & 0xff == 0 and L.OPT_LAZY & (L.OPT_ADAM | L.OPT_RMSPROP | L.OPT_ADADELTA) == 0


def test_lazy_optimizers_carry_tf_defaults():
    from tlsan_amd import _lib as L
    from tlsan_amd.model import LAZY_OPTIMIZERS, OPTIMIZERS
    assert set(LAZY_OPTIMIZERS) == {"lazy_adam", "lazy_rmsprop", "lazy_adadelta"}
    assert OPTIMIZERS["lazy_adam"] == (L.OPT_ADAM | L.OPT_LAZY, 0.9, 0.999, 1e-8)
    assert OPTIMIZERS["lazy_rmsprop"] == (L.OPT_RMSPROP | L.OPT_LAZY, 0.9, 0.0, 1e-10)
    assert OPTIMIZERS["lazy_adadelta"] == (L.OPT_ADADELTA | L.OPT_LAZY, 0.95, 0.0, 1e-8)
    for name in ("adam", "rmsprop", "adadelta"):           # the same constants as the dense forms
        assert OPTIMIZERS["lazy_" + name][1:] == OPTIMIZERS[name][1:]
        assert OPTIMIZERS["lazy_" + name][0] == OPTIMIZERS[name][0] | L.OPT_LAZY


def test_lazy_kinds_are_refused_without_a_launch():
    L, lib = _lib()
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
        opt = L.Optimizer(kind, 1, 0.9, 0.999, 1e-8, C.addressof(slot) if slots else None,
                          C.addressof(slot) if slots else None)
        return lib.tlsan_train_step_opt(C.byref(dims), C.byref(params), C.byref(b), C.byref(hp), C.byref(opt), None,
                                        state, fake, C.c_size_t(ws_bytes), None)

    for kind in (L.OPT_ADAM, L.OPT_RMSPROP, L.OPT_ADADELTA):
        lk = kind | L.OPT_LAZY
        assert call(lk, L.L2_DENSE) == -4                      # needs the lazy tail
        assert b"TLSAN_L2_LAZY" in lib.tlsan_last_error()
        assert call(lk, L.L2_DENSE, L.NORM_DEDUP) == -4
        assert call(lk, L.L2_LAZY, L.NORM_DEDUP) == -4         # the TF18 norm only
        assert call(lk, L.L2_LAZY, slots=False) == -1          # no slot tables
        assert b"slot1" in lib.tlsan_last_error()
        q = L.Params(*([fake.value] * 8))                      # the table scale must be the state's
        assert call(lk, L.L2_LAZY, params=q) == -1
        assert call(kind, L.L2_LAZY) == -4                     # the dense kinds keep their contract
    assert call(L.OPT_LAZY, L.L2_LAZY) == -1                   # LAZY alone (= with SGD)
    assert b"TLSAN_OPT_LAZY" in lib.tlsan_last_error()
    assert call(L.OPT_LAZY | 7, L.L2_LAZY) == -1


def test_driver_parses_lazy_adam():
    from tlsan_amd import train as T
    from tlsan_amd.model import OPTIMIZERS
    args = T.parse(["--dataset", "x.npz", "--optimizer", "lazy_adam", "--learning_rate", "0.01"])
    assert args.optimizer == "lazy_adam" and args.learning_rate == 0.01 and args.l2_mode == "dense"
    assert args.optimizer in OPTIMIZERS


_SHARDED_REFUSAL = r"""
import os, sys, tempfile
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from tests.helpers import make_config
from tlsan_amd.dist import ShardedModel
init = "file://" + os.path.join(tempfile.mkdtemp(), "pg")
dist.init_process_group("gloo", init_method=init, rank=0, world_size=1)
try:
    for name in ("lazy_adam", "lazy_rmsprop", "lazy_adadelta"):
        try:
            ShardedModel(make_config(optimizer=name), list(range(40)), device="cpu")
        except NotImplementedError as e:
            assert "lazy" in str(e), e
        else:
            raise SystemExit("%s was accepted" % name)
finally:
    dist.destroy_process_group()
print("refused")
"""


def test_sharded_model_refuses_lazy_optimizers():
    """ShardedModel refuses the lazy names beside its optimizer check, ahead of any device work (a world-1 gloo group in
    a child process)."""
    r = subprocess.run([sys.executable, "-c", _SHARDED_REFUSAL, ROOT], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr

"""Lazy Adam / RMSProp / Adadelta on the sharded step without a GPU: the new entry points in the header and the library,
their argument checks (refused before any launch, on pointers that are never dereferenced), the workspace query and the
sharded driver's switches."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tlsan_shard_apply_lazy_opt", "tlsan_shard_apply_lazy_opt_workspace", "tlsan_shard_cate_use")


def _lib():
    from tlsan_amd import _lib as L
    return L, L.load()


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "tlsan.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.tlsan_abi_version() == 15


def test_workspace_query_is_positive_and_monotone():
    L, lib = _lib()
    ws = lib.tlsan_shard_apply_lazy_opt_workspace
    assert ws(0, 1) > 0
    last = 0
    for n_recv in (0, 1, 16, 17, 1000, 100_000, 5_000_000):
        row = [ws(n_recv, Cn) for Cn in (1, 16, 17, 801, 100_000)]
        assert all(x > 0 for x in row) and row == sorted(row), (n_recv, row)
        assert row[0] >= last
        last = row[0]
    for Cn in (1, 801):
        col = [ws(n, Cn) for n in (0, 1, 16, 17, 1000, 100_000, 5_000_000)]
        assert col == sorted(col), (Cn, col)


def _call(lib, L, **kw):
    """tlsan_shard_apply_lazy_opt on fake pointers: every call of this file is refused by the argument checks"""
    fake = 0x1000
    a = dict(shard=fake, ld=76, cI=100, R=250, W=76, reg_item=32, reg_user=42, vals=fake, ldv=76, rows=fake, n_recv=10,
             src_off=(C.c_int32 * 17)(0, 10), G=1, slots64=fake, stamp=1, gscale=1.0, step_dev=fake, reg=1e-3, cate_emb=fake,
             C=20, dc=32, g_cate=fake, cate_use=fake, sumsq_out=fake, sumsq_f32=None, kind=L.OPT_ADAM, slots=[fake] * 4,
             scale=None, step=1, opt_null=False, lr=0.01, ws=fake, ws_bytes=1 << 40)
    a.update(kw)
    s = a["slots"]
    opt = L.ShardOptimizer(a["kind"], a["step"], 0.9, 0.999, 1e-8, s[0], s[1], s[2], s[3], None, None, a["scale"])
    rc = lib.tlsan_shard_apply_lazy_opt(a["shard"], a["ld"], a["cI"], a["R"], a["W"], a["reg_item"], a["reg_user"], a["vals"],
                                        a["ldv"], a["rows"], a["n_recv"], a["src_off"], a["G"], a["slots64"], a["stamp"],
                                        a["gscale"], a["step_dev"], a["reg"], a["cate_emb"], a["C"], a["dc"], a["g_cate"],
                                        a["cate_use"], a["sumsq_out"], a["sumsq_f32"], None if a["opt_null"] else C.byref(opt),
                                        a["lr"], a["ws"], C.c_size_t(a["ws_bytes"]), None)
    return rc, lib.tlsan_last_error().decode()


@pytest.mark.parametrize("name", ["shard", "slots64", "step_dev", "cate_emb", "g_cate", "cate_use", "sumsq_out", "src_off",
                                  "vals", "rows"])
def test_null_pointers_are_refused(name):
    L, lib = _lib()
    rc, msg = _call(lib, L, **{name: None})
    assert rc == -1 and "NULL" in msg, (name, rc, msg)


def test_optimizer_block_is_checked_without_a_launch():
    L, lib = _lib()
    rc, msg = _call(lib, L, opt_null=True)
    assert rc == -1 and "NULL" in msg
    for kind in (L.OPT_SGD, L.OPT_SGD | L.OPT_LAZY, 7):
        rc, msg = _call(lib, L, kind=kind)
        assert rc == -1 and "kind" in msg, (kind, rc, msg)
    for k, slot in enumerate(("shard_s1", "shard_s2", "cate_s1", "cate_s2")):      # the message names the missing slot
        for kind in (L.OPT_ADAM, L.OPT_RMSPROP | L.OPT_LAZY, L.OPT_ADADELTA):
            slots = [0x1000] * 4
            slots[k] = None
            rc, msg = _call(lib, L, kind=kind, slots=slots)
            assert rc == -1 and slot in msg, (slot, rc, msg)
    rc, msg = _call(lib, L, step=0)                                                # Adam's step counts from 1
    assert rc == -1 and "step" in msg
    rc, msg = _call(lib, L, scale=0x1000)                                          # the stored values only: P != 1 is refused
    assert rc == -4 and "scale" in msg, (rc, msg)


def test_shape_limits_are_refused_as_the_siblings_do():
    L, lib = _lib()
    rc, msg = _call(lib, L, W=260, ld=260, ldv=260)
    assert rc == -4 and "256" in msg and "260" in msg, (rc, msg)
    rc, msg = _call(lib, L, G=17)
    assert rc == -4 and "16" in msg and "17" in msg, (rc, msg)
    rc, msg = _call(lib, L, W=74, ld=76)                                           # not a multiple of 4
    assert rc == -4
    rc, msg = _call(lib, L, stamp=0)
    assert rc == -4 and "stamp" in msg
    rc, msg = _call(lib, L, ws_bytes=8)
    assert rc == -2 and "workspace" in msg
    rc, msg = _call(lib, L, src_off=(C.c_int32 * 17)(0, 9))                        # offsets that do not end at n_recv
    assert rc == -1 and "src_off" in msg


def test_cate_use_refuses_bad_arguments():
    L, lib = _lib()
    fake = 0x1000
    good = dict(cate_c=fake, n=100, u_cate=fake, B=16, C=20, use=fake)
    for bad in (dict(use=None), dict(cate_c=None), dict(u_cate=None), dict(C=0), dict(n=-1), dict(B=-1),
                dict(n=2 ** 31 - 8, B=16)):
        a = dict(good, **bad)
        rc = lib.tlsan_shard_cate_use(a["cate_c"], a["n"], a["u_cate"], a["B"], a["C"], a["use"], None)
        assert rc == -1 and b"tlsan_shard_cate_use" in lib.tlsan_last_error(), bad


def test_sharded_driver_parses_the_lazy_names():
    from tlsan_amd import train as T
    from tlsan_amd.model import LAZY_OPTIMIZERS
    for name in LAZY_OPTIMIZERS:
        args = T.parse(["--dataset", "x.npz", "--sharded", "1", "--optimizer", name])
        assert args.sharded == 1 and args.optimizer == name and args.static_rows == 0
    args = T.parse(["--dataset", "x.npz", "--sharded", "1", "--optimizer", "lazy_rmsprop", "--learning_rate", "0.02"])
    assert args.optimizer == "lazy_rmsprop" and args.learning_rate == 0.02


_DRIVER_REFUSAL = r"""
import os, sys, tempfile
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from tlsan_amd import train as T
tmp = tempfile.mkdtemp()
dist.init_process_group("gloo", init_method="file://" + os.path.join(tmp, "pg"), rank=0, world_size=1)
try:
    ds = os.path.join(sys.argv[1], "tests", "golden", "packed_clothing.npz")
    argv = ["--dataset", ds, "--sharded", "1", "--optimizer", "lazy_adam", "--static_rows", "1", "--quiet",
            "--model_dir", os.path.join(tmp, "ck")]
    try:
        T.train_sharded(T.parse(argv))
    except NotImplementedError as e:
        assert "static_rows" in str(e) and "lazy_adam" in str(e), e
    else:
        raise SystemExit("accepted")
    assert not os.path.exists(os.path.join(tmp, "ck"))        # refused before anything was set up
finally:
    dist.destroy_process_group()
print("refused")
"""


def test_sharded_driver_refuses_static_rows_with_a_lazy_name():
    """--static_rows is the lazy-L2 SGD step's form: refused for the lazy optimizers ahead of any device work (a world-1
    gloo group in a child process)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _DRIVER_REFUSAL, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr

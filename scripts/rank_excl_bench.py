#!/usr/bin/env python3
"""Cost of the filtered full ranking (tlsan_eval_ranks_excl: the all-items count + k_excl_ahead on the rows' exclusion
lists) against the unfiltered ranking pass (tlsan_eval_ranks) of the PARENT commit's library, alternating in one process.

Shape: the Electronics test set's size (synth.make_config("electronics"): 39 991 rows, I = 22 048, d = 128) in the
driver's launches of 4096 rows, with synthetic seen lists of 16 and of 90 distinct items per row (sorted, one CSR per
launch, built before the clock starts).  Both passes get the same u_t, labels, tables and workspace; the parent's library
is loaded next to this tree's (--parent-lib: a build of the parent commit in a second directory; without it the
unfiltered pass runs in this tree's library and the table says so).  Also the whole Model.label_ranks pass (forward +
ranking) without and with a SeenItems holder, whose per-launch exclusion CSR is built by torch ops inside the clock.
Times are host clocks around synchronised loops, both alternating rounds listed; the kernel's own time comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script (--quick).  Algorithmic bytes of the correction:
B * len * (d_i * e + d_c * e + 12) (item row, category row, category id, bias and list entry per listed item), e = 4.

    python scripts/rank_excl_bench.py [--parent-lib ab_old/tlsan_amd/libtlsan_hip.so] [--quick] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tlsan_amd import _lib as L  # noqa: E402
from tlsan_amd import synth  # noqa: E402
from tlsan_amd.model import Model, SeenItems  # noqa: E402

LENS = (16, 90)


def timed(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def parent_library(path):
    lib = C.CDLL(path)
    lib.tlsan_abi_version.restype = C.c_int
    if lib.tlsan_abi_version() != L.ABI_VERSION:
        raise RuntimeError("parent library: ABI %d, this tree %d" % (lib.tlsan_abi_version(), L.ABI_VERSION))
    lib.tlsan_eval_ranks.argtypes = L.load().tlsan_eval_ranks.argtypes
    lib.tlsan_eval_ranks.restype = C.c_int
    return lib


def row_lists(B, I, n, seed, device):
    """[B, n] int32: n distinct items per row, ascending."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    parts = []
    for lo in range(0, B, 4096):          # (a [4096, I] draw at a time)
        pick = torch.rand(min(4096, B - lo), I, generator=g, device=device).argsort(1)[:, :n]
        parts.append(pick.sort(1).values.to(torch.int32))
    return torch.cat(parts).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libtlsan_hip.so built from the parent commit")
    ap.add_argument("--quick", action="store_true", help="few iterations (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = 2 if a.quick else 20
    cfg = synth.make_config("electronics")
    rows, chunk, I = 39991, 4096, cfg["item_count"]
    m = Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")
    new = m.lib
    old = parent_library(a.parent_lib) if a.parent_lib else new
    sizes = [min(chunk, rows - lo) for lo in range(0, rows, chunk)]
    dbs = [m.device_batch(synth.make_batches(cfg, 1, s, seed=20 + i, test=True)[0], is_test=True) for i, s in enumerate(sizes)]
    uts = [m.forward(db, is_test=True, want_u_t=True)[2] for db in dbs]
    ws = m._workspace(chunk, 0)
    st = m._stream()
    outs = [torch.empty(3, s, dtype=torch.int32, device=m.device) for s in sizes]
    lists = {ln: [row_lists(s, I, ln, 100 * ln + i, m.device) for i, s in enumerate(sizes)] for ln in LENS}
    offs = {ln: [torch.arange(0, (s + 1) * ln, ln, dtype=torch.int32, device=m.device) for s in sizes] for ln in LENS}

    def unfiltered():
        for db, ut, o in zip(dbs, uts, outs):
            L.check(old.tlsan_eval_ranks(C.byref(m.dims), C.byref(m.cparams), ut.data_ptr(), db.i.data_ptr(), db.B,
                                         o[0].data_ptr(), ws.data_ptr(), ws.numel(), st), "tlsan_eval_ranks")

    def filtered(ln):
        for db, ut, o, off, ids in zip(dbs, uts, outs, offs[ln], lists[ln]):
            L.check(new.tlsan_eval_ranks_excl(C.byref(m.dims), C.byref(m.cparams), ut.data_ptr(), db.i.data_ptr(), db.B,
                                              off.data_ptr(), ids.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                                              o[2].data_ptr(), ws.data_ptr(), ws.numel(), st), "tlsan_eval_ranks_excl")

    # the two libraries agree on the unfiltered ranks, and the correction is what it says
    unfiltered()
    want = [o[0].clone() for o in outs]
    for ln in LENS:
        filtered(ln)
        assert all(torch.equal(o[0], w) for o, w in zip(outs, want))
        assert all(int((o[1] > o[0]).sum()) == 0 and int(o[2].min()) >= ln - 1 for o in outs)
    res = dict(shape="electronics", rows=rows, chunk=chunk, I=I, d=cfg["hidden_units"], iterations=n,
               parent_lib=bool(a.parent_lib), rounds=[])
    for rnd in range(2):
        r = dict(unfiltered_pass_us=timed(unfiltered, n) * 1e6)
        for ln in LENS:
            r["filtered_pass_us_len%d" % ln] = timed(lambda: filtered(ln), n) * 1e6
        res["rounds"].append(r)
        print("round %d: unfiltered (%s library) %8.1f us | " % (rnd + 1, "parent" if a.parent_lib else "this", r["unfiltered_pass_us"])
              + " | ".join("filtered, %d items per row %8.1f us (+%.1f %%)"
                           % (ln, r["filtered_pass_us_len%d" % ln],
                              100 * (r["filtered_pass_us_len%d" % ln] / r["unfiltered_pass_us"] - 1)) for ln in LENS), flush=True)
    # the whole evaluation pass of the model: forward + ranking, the exclusion CSR built per launch by torch ops
    U = cfg["user_count"]
    for ln in LENS:
        ids = row_lists(U, I, ln, 7 + ln, m.device).cpu().numpy()
        holder = SeenItems(np.arange(0, (U + 1) * ln, ln), ids.reshape(-1), m.device)
        for rnd in range(2):
            t0 = timed(lambda: [m.label_ranks(db) for db in dbs], n) * 1e6
            t1 = timed(lambda: [m.label_ranks(db, exclude=holder) for db in dbs], n) * 1e6
            res["rounds"][rnd]["model_pass_us_beside_len%d" % ln] = t0
            res["rounds"][rnd]["model_filtered_pass_us_len%d" % ln] = t1
            print("Model.label_ranks pass, round %d: unfiltered %8.1f us | SeenItems of %d items per user (+ the row's input) "
                  "%8.1f us" % (rnd + 1, t0, ln, t1), flush=True)
    for ln in LENS:
        nbytes = chunk * ln * (4 * cfg["itemid_embedding_size"] + 4 * cfg["cateid_embedding_size"] + 12)
        res["excl_bytes_len%d" % ln] = nbytes
        print("algorithmic bytes of k_excl_ahead, %d rows x %d items: %.1f MB" % (chunk, ln, nbytes / 1e6))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

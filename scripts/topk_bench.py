#!/usr/bin/env python3
"""Cost of the top-K recommendation (Model.recommend: tlsan_eval_topk) against the all-items ranking it extends
(Model.label_ranks: tlsan_eval_ranks) on the same batches, alternating in one process.  Electronics-scale synthetic
shape (synth.make_config("electronics"), I = 22 048, d = 128) at B = 4096, K in {1, 10, 50, 256}, with no exclusion
and with exclude="history"; one large-table point (I = 300 000, d = 256: [I, d] above the dense-matrix limit, the
gather form).  Times are host clocks around a synchronised loop and include the forward that produces u_t (both
paths run it); kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--quick).

    python scripts/topk_bench.py [--quick] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tlsan_amd import synth  # noqa: E402
from tlsan_amd.model import Model  # noqa: E402

PEAK_F32_MATRIX = 157.3e12   # MI355X fp32 MFMA peak (spec)


def timed(fn, batches, n):
    for s in range(3):
        fn(batches[s % len(batches)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(n):
        fn(batches[s % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def run(name, cfg, B, ks, n, out):
    icl = synth.item_cate_list(cfg)
    m = Model(cfg, icl, l2_mode="lazy", init="device")
    tb = [m.device_batch(b, is_test=True) for b in synth.make_batches(cfg, 2, B, seed=9, test=True)]
    flop = 2.0 * B * cfg["item_count"] * cfg["hidden_units"]
    fwd = timed(lambda db: m.forward(db, is_test=True, want_u_t=True), tb, n)
    for k in ks:
        for ex in (None, "history"):
            # alternate: ranks, top-K, ranks, top-K ... (two rounds each, the better of the two)
            r_t, k_t = [], []
            for _ in range(2):
                r_t.append(timed(m.label_ranks, tb, n))
                k_t.append(timed(lambda db: m.recommend(db, k, exclude=ex), tb, n))
            r, t = min(r_t), min(k_t)
            row = dict(shape=name, I=cfg["item_count"], d=cfg["hidden_units"], B=B, K=k, exclude=ex or "none",
                       forward_us=fwd * 1e6, label_ranks_us=r * 1e6, recommend_us=t * 1e6, ratio=t / r,
                       recommend_tflops_excl_forward=flop / max(t - fwd, 1e-9) / 1e12,
                       label_ranks_tflops_excl_forward=flop / max(r - fwd, 1e-9) / 1e12)
            out.append(row)
            print("%-12s B=%d K=%3d exclude=%-7s forward %7.1f us | label_ranks %7.1f us | recommend %7.1f us (x%.2f) | "
                  "scoring+selection %.1f TFLOP/s (%.0f %% of fp32 matrix peak), ranking %.1f TFLOP/s"
                  % (name, B, k, ex or "none", fwd * 1e6, r * 1e6, t * 1e6, t / r, row["recommend_tflops_excl_forward"],
                     100 * row["recommend_tflops_excl_forward"] * 1e12 / PEAK_F32_MATRIX,
                     row["label_ranks_tflops_excl_forward"]), flush=True)
    del m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quick", action="store_true", help="few iterations (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = 3 if a.quick else 20
    out = []
    run("electronics", synth.make_config("electronics"), 4096, (1, 10, 50, 256), n, out)
    big = synth.make_config("electronics", hidden_units=256, itemid_embedding_size=128, userid_embedding_size=128,
                            cateid_embedding_size=128, item_count=300000)
    run("large-table", big, 4096, (10, 50), n, out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

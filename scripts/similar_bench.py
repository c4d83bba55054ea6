#!/usr/bin/env python3
"""Cost of the similar-items lists (Model.similar_items: tlsan_item_vectors + tlsan_similar_topk) against the top-K
selection whose tile loop they share (tlsan_eval_topk on a fixed u_t: no forward on either side), alternating in one
process.  Electronics-scale synthetic shape (synth.make_config("electronics"), I = 22 048, d = 128) at Q = B = 4096,
K in {10, 100}, cosine and dot.  Times are host clocks around a synchronised loop; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--quick, one --metric at a time: both metrics run the same
instantiation of k_similar_topk, so a trace of both would average them):

    python scripts/ab.py --rounds 1 --trace --top 8 -- python scripts/similar_bench.py --quick --metric cosine
    python scripts/similar_bench.py [--quick] [--metric cosine|dot|both] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tlsan_amd import synth  # noqa: E402
from tlsan_amd.model import Model, eval_topk  # noqa: E402


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quick", action="store_true", help="few iterations (for a kernel-trace run)")
    ap.add_argument("--metric", default="both", choices=["cosine", "dot", "both"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = 3 if a.quick else 20
    cfg = synth.make_config("electronics")
    I, d, B = cfg["item_count"], cfg["hidden_units"], 4096
    m = Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")
    g = torch.Generator(device="cpu").manual_seed(9)
    items = torch.randint(0, I, (B,), generator=g).numpy()
    ut = torch.randn(B, d, generator=g).to(m.device)
    flop = 2.0 * B * I * d
    out = []
    for k in (10, 100):
        for metric in (("cosine", "dot") if a.metric == "both" else (a.metric,)):
            # alternate: top-K, similar, top-K, similar (two rounds each, the better of the two)
            t_t, s_t = [], []
            for _ in range(2):
                t_t.append(timed(lambda: eval_topk(m.lib, m.dims, m.cparams, ut, B, k, (None, None), 1, 0, m._topk_workspace,
                                                   m._stream()), n))
                s_t.append(timed(lambda: m.similar_items(items, k, metric=metric), n))
            t, s = min(t_t), min(s_t)
            out.append(dict(I=I, d=d, Q=B, K=k, metric=metric, eval_topk_us=t * 1e6, similar_items_us=s * 1e6, ratio=s / t,
                            similar_tflops=flop / s / 1e12, eval_topk_tflops=flop / t / 1e12))
            print("electronics Q=B=%d K=%3d %-6s eval_topk %7.1f us (%.1f TFLOP/s) | similar_items %7.1f us (%.1f TFLOP/s) x%.2f"
                  % (B, k, metric, t * 1e6, flop / t / 1e12, s * 1e6, flop / s / 1e12, s / t), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the sampled evaluation (Model.sampled_ranks: forward + tlsan_sample_negatives + tlsan_score_candidates +
tlsan_candidate_ranks) against the all-items ranking (Model.label_ranks: forward + tlsan_eval_ranks) on the same rows,
alternating in one process, and of the candidate scoring kernel alone.

Shapes: the Electronics test set's size (synth.make_config("electronics"): 39 991 rows, I = 22 048, d = 128) in the
driver's launches of 4096 rows, at N = 100 and N = 1000 negatives; a 5 M-item d = 256 table (item rows 2.56 GB, far
beyond the 256 MiB Infinity Cache) at B = 4096, N = 100 (sampled pass and scoring only: its all-items ranking is
~10 TFLOP per call).  Times are host clocks around synchronised loops; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (--quick).  The scoring's algorithmic bytes are
B·C·(d_i·e + d_c·e + 4 + 4 + 4) + B·d·4 (item row, category row, category id, bias and candidate id per candidate, plus
u_t), e = 4 (fp32 tables).

    python scripts/cand_bench.py [--quick] [--json out.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tlsan_amd import synth  # noqa: E402
from tlsan_amd.model import Model, exclusion_csr, sample_negatives, score_candidates  # noqa: E402

HBM_GBS = 6300.0   # MI355X achievable HBM read rate (float4 copy), GB/s


def timed(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def score_bytes(cfg, B, Cn):
    return B * Cn * (4 * cfg["itemid_embedding_size"] + 4 * cfg["cateid_embedding_size"] + 12) + B * cfg["hidden_units"] * 4


def run(name, cfg, rows, chunk, ns, n, out, full_ranking=True):
    icl = synth.item_cate_list(cfg)
    m = Model(cfg, icl, l2_mode="lazy", init="device")
    sizes = [min(chunk, rows - lo) for lo in range(0, rows, chunk)]
    dbs = [m.device_batch(synth.make_batches(cfg, 1, s, seed=20 + i, test=True)[0], is_test=True)
           for i, s in enumerate(sizes)]
    row0 = [sum(sizes[:i]) for i in range(len(sizes))]
    fwd = timed(lambda: [m.forward(db, is_test=True, want_u_t=True) for db in dbs], n)
    ranks_t = None
    for N in ns:
        s_t, r_t = [], []
        for _ in range(2):     # alternate: full ranking, sampled, full ranking, sampled (the better of each)
            if full_ranking:
                r_t.append(timed(lambda: [m.label_ranks(db) for db in dbs], n))
            s_t.append(timed(lambda: [m.sampled_ranks(db, N, row0=r0) for db, r0 in zip(dbs, row0)], n))
        if full_ranking:
            ranks_t = min(r_t)
        samp = min(s_t)
        # the kernels alone on the first chunk: sampling, scoring of [label | negatives]
        db = dbs[0]
        _, _, ut, _ = m.forward(db, is_test=True, want_u_t=True)
        st = m._stream()
        excl = exclusion_csr(db, "history", cfg["item_count"])
        neg_t = timed(lambda: sample_negatives(m.lib, cfg["item_count"], db.i, N, 1234, 0, excl, st), n)
        neg = sample_negatives(m.lib, cfg["item_count"], db.i, N, 1234, 0, excl, st)
        cand = torch.cat([db.i.view(-1, 1), neg], 1).contiguous()
        sc = torch.empty(cand.shape, dtype=torch.float32, device=m.device)
        score_t = timed(lambda: score_candidates(m.lib, m.dims, m.cparams, ut, cand, 1, 0, st, scores=sc), n)
        nbytes = score_bytes(cfg, db.B, N + 1)
        row = dict(shape=name, I=cfg["item_count"], d=cfg["hidden_units"], rows=rows, chunk=chunk, N=N,
                   forward_pass_us=fwd * 1e6, sampled_pass_us=samp * 1e6,
                   full_ranking_pass_us=None if ranks_t is None else ranks_t * 1e6,
                   sample_call_us=neg_t * 1e6, score_call_us=score_t * 1e6, score_bytes=nbytes,
                   score_gbs=nbytes / score_t / 1e9)
        out.append(row)
        print("%-12s rows=%d N=%4d | forward %8.1f us | sampled pass %8.1f us | full ranking %s | one launch of %d rows: "
              "sample %7.1f us, score %7.1f us = %.0f GB/s (%.0f %% of HBM)"
              % (name, rows, N, fwd * 1e6, samp * 1e6, "-" if ranks_t is None else "%8.1f us" % (ranks_t * 1e6),
                 db.B, neg_t * 1e6, score_t * 1e6, row["score_gbs"], 100 * row["score_gbs"] / HBM_GBS), flush=True)
    del m
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quick", action="store_true", help="few iterations (for a kernel-trace run)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = 2 if a.quick else 10
    out = []
    run("electronics", synth.make_config("electronics"), 39991, 4096, (100, 1000), n, out)
    big = synth.make_config("electronics", hidden_units=256, itemid_embedding_size=128, userid_embedding_size=128,
                            cateid_embedding_size=128, item_count=5000000)
    run("5M-items", big, 4096, 4096, (100,), n, out, full_ranking=False)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

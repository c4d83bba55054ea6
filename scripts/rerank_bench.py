#!/usr/bin/env python3
"""Cost of the re-ranking stage of a diversified list (tlsan_rerank, k_rerank) beside the call that makes its pool,
Model.recommend(k = N) on the same rows, alternating in one process: B = 4096 rows, N in {64, 256}, K in {10, 100},
d in {64, 128, 256} (electronics-scale synthetic table, I = 22 048, 673 categories), theta = 0.5 and no cap, so that every one of the K
steps runs (a cap ends a row early when its pool holds few categories).  Times are
device events around the call (one launch: the kernel and its launch), the median of the timed calls; the pool's vectors,
inverse norms and categories are staged once outside the timed window, as Model.recommend stages them per chunk.

    python scripts/rerank_bench.py [--out profiles/rerank.md]     every d as a step of scripts/steps.py, then the report
    python scripts/rerank_bench.py --measure D --json FILE        one d (a step of the above)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
B, THETA, CAP = 4096, 0.5, 0
SHAPES = [(N, K) for N in (64, 256) for K in (10, 100) if K <= N]


def median_ms(fn, n):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def measure(d, path, n):
    import torch
    from tlsan_amd import model as M
    from tlsan_amd import synth
    cfg = synth.make_config("electronics", hidden_units=d, itemid_embedding_size=d // 2, userid_embedding_size=d // 2,
                            cateid_embedding_size=d // 2)
    m = M.Model(cfg, synth.item_cate_list(cfg), init="device")
    batch = synth.make_batches(cfg, 1, batch_size=B, test=True)[0]
    db = m.device_batch(batch, is_test=True)
    out = []
    for N, K in SHAPES:
        pid, psc = m.recommend(db, N, exclude="history")
        rows = min(B, M.rerank_chunk(N, d))
        flat = pid[:rows].reshape(-1)
        vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, flat, 1, 0, m._stream())
        cate = m.item_cate[flat.clamp(min=0).long()]
        ids = torch.empty(rows, K, dtype=torch.int32, device=m.device)
        sc = torch.empty(rows, K, dtype=torch.float32, device=m.device)
        kernel = lambda: M.rerank(m.lib, pid[:rows], psc[:rows], vec, inv, cate, K, THETA, CAP, ids, sc, m._stream())
        pool = lambda: m.recommend(db, N, exclude="history")
        whole = lambda: m.recommend(db, K, exclude="history", diversity=THETA, per_category=CAP, pool=N)
        t_k, t_p, t_w = [], [], []
        for _ in range(2):                       # alternate; the better of the two rounds
            t_k.append(median_ms(kernel, n))
            t_p.append(median_ms(pool, n))
            t_w.append(median_ms(whole, n))
        assert int((ids < 0).sum().item()) == 0      # every row ran its K steps
        out.append(dict(d=d, N=N, K=K, rows=rows, rerank_ms=min(t_k), rerank_us_per_row=1e3 * min(t_k) / rows,
                        recommend_pool_ms=min(t_p), recommend_diversified_ms=min(t_w)))
        print(json.dumps(out[-1]), flush=True)
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=out), f, indent=1)


def digest(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def report(out, log_dir, n):
    from steps import log_path, run_steps
    py = sys.executable
    steps = [("registers", [py, os.path.join(ROOT, "scripts", "kernel_registers.py"), "--all", "tlsan_rerank"], None, 300, ROOT)]
    steps += [("d%d" % d, [py, os.path.abspath(__file__), "--measure", d, "--json", os.path.join(log_dir, "d%d.json" % d),
                           "--iters", n], None, 420, ROOT) for d in (64, 128, 256)]
    rc = run_steps(steps, log_dir)
    if rc:
        return rc
    csrc = os.path.join(ROOT, "tlsan_amd", "csrc")
    res = [json.load(open(os.path.join(log_dir, "d%d.json" % d))) for d in (64, 128, 256)]
    hipcc = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
    lines = ["# Diversified lists: `k_rerank` beside the call that makes its pool", "",
             "Made by `python scripts/rerank_bench.py` (steps of `scripts/steps.py`, one per d).  Build: `libtlsan_hip.so` sha256 `%s`,"
             % digest([os.path.join(ROOT, "tlsan_amd", "libtlsan_hip.so")]),
             "`tlsan_rerank.h` + `tlsan_rerank.hip` sha256 `%s`, %s; device %s." % (
                 digest([os.path.join(csrc, "tlsan_rerank.h"), os.path.join(csrc, "tlsan_rerank.hip")]),
                 hipcc[0] if hipcc else "hipcc unknown", res[0]["device"]), "",
             "## Registers (`scripts/kernel_registers.py --all tlsan_rerank`; `k_rerank<D, threads>`, occupancy in waves per SIMD)", "",
             "```", open(log_path(log_dir, "registers")).read().strip(), "```", "",
             "No instantiation spills (scratch = 0).  1024 threads are 4 waves per SIMD: at most 128 registers per lane.", "",
             "## Times", "",
             "B = %d rows of an electronics-scale table (I = 22 048), theta = %.1f, per_category = %d, exclude = history; device events,"
             % (B, THETA, CAP),
             "median of %d calls, the better of two alternating rounds.  `rerank`: the `tlsan_rerank` call alone on staged inputs"
             % n,
             "(`rows` of them: one chunk of the 256 MB staging rule); `pool`: `Model.recommend(k = N)`, forward and top-N selection;",
             "`diversified`: `Model.recommend(k = K, diversity, per_category, pool = N)`, everything (pool, vectors, categories, re-ranking",
             "of every chunk).  Without a cap every row runs its K steps.", "",
             "| d | N | K | rows | rerank ms | rerank us / row | pool ms | diversified ms |", "|---|---|---|---|---|---|---|---|"]
    for r in res:
        for x in r["rows"]:
            lines.append("| %d | %d | %d | %d | %.3f | %.3f | %.3f | %.3f |" % (
                x["d"], x["N"], x["K"], x["rows"], x["rerank_ms"], x["rerank_us_per_row"], x["recommend_pool_ms"],
                x["recommend_diversified_ms"]))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", type=int, default=0, choices=[0, 64, 128, 256])
    ap.add_argument("--json", default=None)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank.md"))
    ap.add_argument("--log_dir", default=os.path.join(ROOT, "measure_out", "rerank"))
    a = ap.parse_args()
    if a.measure:
        measure(a.measure, a.json, a.iters)
        return 0
    return report(a.out, a.log_dir, a.iters)


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Cost and recall of the clustered item index (recommend's index= with probes=) at d = 128, B = 4096, K = 10 against the
exact recommend() -- the scan of every item, the parent commit's path -- timed in the same process, interleaved.

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    synth_this                       5 M items in 200 even categories (synth.py; half of an item's vector is its category's
                                     embedding, so the vectors carry category structure): for nlists in 256, 1024, 4096 the
                                     build, then three rounds of [exact recommend, probes = 1, 2, 4, 8, 16, 32]
    small_this                       bench.py's Electronics tables: 63 001 items in 801 categories, the same sweep
    bench_this_<r>, bench_parent_<r> bench.py's fp32 leg (ms_per_step_p50) -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one);
without it the parent's steps are left out.  Times are host clocks around a synchronised loop of --iters calls behind a
warm-up; recommend's include the forward that produces u_t.  recall@10 is cluster.recall of the approximate ids against
the exact ones over the B rows.

    python scripts/cluster_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/cluster]
    python scripts/cluster_bench.py --part synth|small"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, K = 4096, 10
NLISTS = (256, 1024, 4096)
PROBES = (1, 2, 4, 8, 16, 32)


def timed(fn, n):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def model_of(shape):
    from tlsan_amd import synth
    from tlsan_amd.model import Model
    kw = dict(item_count=5000000, cate_count=200) if shape == "synth" else {}
    cfg = synth.make_config("electronics", **kw)
    return cfg, Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")


def part(shape, n, rounds, nlists_sweep):
    import torch
    from tlsan_amd import synth
    from tlsan_amd.cluster import recall
    cfg, m = model_of(shape)
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    out = lambda case, **kw: print(json.dumps(dict(part=shape, case=case, **kw)), flush=True)
    exact = m.recommend(db, K)[0]
    for nlists in nlists_sweep:
        if nlists > cfg["item_count"]:
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ci = m.cluster_index(nlists)
        torch.cuda.synchronize()
        out("build", nlists=nlists, ms=round((time.perf_counter() - t0) * 1e3, 1), iterations=len(ci.objective),
            max_list=ci.max_list, mean_list=round(ci.mean_list, 1), nonempty=ci.nonempty)
        for p in PROBES:
            out("recall", nlists=nlists, probes=p, recall=round(recall(m.recommend(db, K, index=ci, probes=p)[0], exact), 4))
        for r in range(rounds):                                 # the exact scan and the probes, interleaved
            out("exact", nlists=nlists, round=r, ms=round(timed(lambda: m.recommend(db, K), n), 3))
            for p in PROBES:
                out("query", nlists=nlists, probes=p, round=r, ms=round(timed(lambda: m.recommend(db, K, index=ci, probes=p), n), 3))
        del ci


def lines_of(path, key):
    rows = []
    with open(path, errors="replace") as f:
        for line in f:
            if line.startswith("{") and key in line:
                rows.append(json.loads(line))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["synth", "small"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nlists", default=",".join(str(x) for x in NLISTS))
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--lists", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "cluster"))
    a = ap.parse_args()
    if a.part:
        return part(a.part, a.iters, a.rounds, [int(x) for x in a.nlists.split(",")])
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters, "--rounds", a.rounds, "--nlists", a.nlists]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    steps = []
    if a.lists:
        steps += [("synth_this", me + ["--part", "synth"], {}, 600, ROOT), ("small_this", me + ["--part", "small"], {}, 300, ROOT)]
    for r in range(a.rounds if a.bench else 0):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    med = lambda v: sorted(v)[len(v) // 2]
    print("B = %d, K = %d; ms: median (min max) of %d interleaved rounds" % (B, K, a.rounds))
    for name in ("synth_this", "small_this") if a.lists else ():
        rows = lines_of(log_path(a.out, name), '"part"')
        for b in (r for r in rows if r["case"] == "build"):
            nl = b["nlists"]
            ex = [r["ms"] for r in rows if r["case"] == "exact" and r["nlists"] == nl]
            print("%-11s nlists %5d  build %9.1f ms (%d iterations)  lists max %d mean %.1f nonempty %d  exact %.3f (%.3f %.3f)"
                  % (name, nl, b["ms"], b["iterations"], b["max_list"], b["mean_list"], b["nonempty"], med(ex), min(ex), max(ex)))
            for p in PROBES:
                q = [r["ms"] for r in rows if r["case"] == "query" and r["nlists"] == nl and r["probes"] == p]
                rec = [r["recall"] for r in rows if r["case"] == "recall" and r["nlists"] == nl and r["probes"] == p][0]
                print("%-11s nlists %5d  probes %2d  %9.3f (%.3f %.3f)  x%.1f  recall@%d %.4f"
                      % (name, nl, p, med(q), min(q), max(q), med(ex) / med(q), K, rec))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

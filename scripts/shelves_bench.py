#!/usr/bin/env python3
"""Cost of a page of category shelves (Model.shelves) at d = 128, B = 4096, S = 8, m = 10, against the only exact way the
parent commit offers -- one recommend(category=full(c), index=idx) per category with items, run on the parent's library --
and against the work floor, recommend(S * m) without an index (one full scan), on the three tables of
profiles/category_index.md.

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out), fresh processes, this build alternating with the parent's:

    <table>_this_<r>     forward, the floor, shelves at the production thresholds (and, with --sweep 1 in round 0, at the
                         thresholds of SWEEP), recommend(category=, index=) of the row's own department
    <table>_parent_<r>   forward, the floor, the loop over the categories, recommend(category=, index=)
    bench_<side>_<r>     bench.py's fp32 leg (ms_per_step_p50) -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one);
without it the parent's steps are left out.  Times are host clocks around a synchronised loop of --iters calls behind a
warm-up (the loop over the categories: one warm-up pass, one timed pass); all of them include the forward that produces u_t.

    python scripts/shelves_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/shelves]
    python scripts/shelves_bench.py --part even|small|skewed"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, S, M = 4096, 8, 10
TABLES = ("even", "small", "skewed")
SWEEP = ((4096, 16384), (16384, 65536), (65536, 262144), (262144, 1048576), (65536, 0), (65536, 1 << 30))


def part(shape, n, sweep):
    import numpy as np
    import torch
    from catidx_bench import model_of, timed
    from tlsan_amd import synth
    from tlsan_amd.model import shelves_plan, shelves_thresholds
    cfg, m = model_of(shape)
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    out = lambda case, ms, **kw: print(json.dumps(dict(part=shape, case=case, ms=round(ms, 3), **kw)), flush=True)
    out("forward", timed(lambda: m.forward(db, is_test=True, want_u_t=True), n))
    out("floor: recommend(%d), no index" % (S * M), timed(lambda: m.recommend(db, S * M), n))
    idx = m.category_index()
    lens = np.diff(idx.list_off.cpu().numpy())
    cate = m.last_item_categories(db)
    out("recommend category index", timed(lambda: m.recommend(db, M, category=cate, index=idx), n))
    if hasattr(m.lib, "tlsan_eval_shelves"):
        seg, big = shelves_thresholds(idx.count, B)

        def geometry(s, b):
            so, _, bo, bs = shelves_plan(lens, s, b)
            return dict(nseg=len(so) - 1, nbig=len(bo) - 1, nbs=len(bs))
        out("shelves", timed(lambda: m.shelves(db, S, M, index=idx), n), seg_items=seg, big_items=big, **geometry(seg, big))
        for s, b in SWEEP if sweep else ():
            out("shelves sweep", timed(lambda: m.shelves(db, S, M, index=idx, seg_items=s, big_items=b), n), seg_items=s,
                big_items=b, **geometry(s, b))
    else:                                                          # the parent's only exact way
        cats = [torch.full((B,), int(c), dtype=torch.int32, device=m.device) for c in np.flatnonzero(lens)]

        def loop():
            for c in cats:
                m.recommend(db, M, category=c, index=idx)
        out("loop over %d categories" % len(cats), timed(loop, 1), lists=len(cats), longest=int(lens.max()))


def lines_of(path, key):
    rows = []
    with open(path, errors="replace") as f:
        for line in f:
            if line.startswith("{") and key in line:
                rows.append(json.loads(line))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=TABLES)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", type=int, default=0, help="1: round 0 of this build also times the thresholds of SWEEP")
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--pages", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "shelves"))
    a = ap.parse_args()
    if a.part:
        return part(a.part, a.iters, a.sweep)
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    steps = []
    for r in range(a.rounds if a.pages else 0):
        for table in TABLES:
            steps += [("%s_%s_%d" % (table, side, r), me + ["--part", table, "--sweep", int(bool(a.sweep and r == 0 and side == "this"))],
                       env, 400, ROOT) for side, env in sides]
    for r in range(a.rounds if a.bench else 0):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    print("B = %d, S = %d, m = %d; ms: median (min max of %d processes)" % (B, S, M, a.rounds))
    for table in TABLES if a.pages else ():
        for side, _ in sides:
            rows = {}
            for r in range(a.rounds):
                for row in lines_of(log_path(a.out, "%s_%s_%d" % (table, side, r)), '"part"'):
                    key = row["case"] + ("" if row["case"] != "shelves sweep" else " %d / %d" % (row["seg_items"], row["big_items"]))
                    rows.setdefault(key, []).append((row["ms"], {k: v for k, v in row.items() if k not in ("part", "case", "ms")}))
            for case, v in rows.items():
                ms = sorted(x[0] for x in v)
                print("%-7s %-6s %-44s %11.3f   (%.3f %.3f)  %s" % (table, side, case, ms[len(ms) // 2], ms[0], ms[-1],
                                                                    json.dumps(v[0][1]) if v[0][1] else ""))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

#!/usr/bin/env python3
"""Cost of the per-category item index (recommend's / similar_items' index=) at d = 128, B = Q = 4096, K = 10, against the
category form without an index, on this build and on the parent commit's library in the same run.

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    even_this_<r>, even_parent_<r>   5 M items in 200 even categories (profiles/scoped.md's shape): recommend(category=),
                                     similar_items(same_category=True) cosine / dot and the plain similar_items on both
                                     sides; on this build also the indexed calls and within= one category
    small_this                       bench.py's Electronics tables: 63 001 items in 801 categories
    skewed_this                      5 M items, 20 categories hold 90 % of them and 2 000 the rest, with the idle
                                     workgroups of the launch (idle_workgroups below: the grid against the list lengths)
    bench_this_<r>, bench_parent_<r> bench.py's fp32 leg (ms_per_step_p50) -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one);
without it the parent's steps are left out.  Times are host clocks around a synchronised loop of --iters calls behind a
warm-up; recommend's include the forward that produces u_t.

    python scripts/catidx_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/catidx]
    python scripts/catidx_bench.py --part even|small|skewed"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, K = 4096, 10


def timed(fn, n):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def eval_slices(ut, n):
    """csrc/tlsan_eval.h"""
    want = (2048 + ut - 1) // ut
    return want if n > want else max(n, 1)


def idle_workgroups(row_lists, list_len):
    """The launch of tlsan_eval_topk_lists for row_lists [B, P] over lists of list_len items -> (workgroups launched,
    workgroups that leave at once: past the real group count, or with a slice that starts past their list's end)."""
    import numpy as np
    rl = np.asarray(row_lists).reshape(len(row_lists), -1)
    N, nlists = rl.size, len(list_len)
    pairs = np.zeros(nlists, np.int64)
    for row in rl:
        for c in set(int(x) for x in row if 0 <= x < nlists and list_len[x] > 0):
            pairs[c] += 1
    nsl = eval_slices((N + 15) // 16, ((int(max(list_len)) + 63) // 64 + 3) // 4)
    grid = (N // 16 + min(nlists, N)) * nsl
    groups = (pairs + 15) // 16
    working = int((groups * np.minimum(nsl, (np.asarray(list_len) + 255) // 256)).sum())
    return grid, grid - working, nsl, int(groups.sum())


def model_of(shape):
    import numpy as np
    from tlsan_amd import synth
    from tlsan_amd.model import Model
    if shape == "small":
        cfg = synth.make_config("electronics")
        return cfg, Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")
    if shape == "even":
        cfg = synth.make_config("electronics", item_count=5000000, cate_count=200)
        return cfg, Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")
    cfg = synth.make_config("electronics", item_count=5000000, cate_count=2020)
    rng = np.random.default_rng(7)
    big = rng.random(5000000) < 0.9
    cate = np.where(big, rng.integers(0, 20, 5000000), rng.integers(20, 2020, 5000000)).astype(np.int32)
    return cfg, Model(cfg, cate, l2_mode="lazy", init="device")


def part(shape, n):
    import numpy as np
    import torch
    from tlsan_amd import synth
    cfg, m = model_of(shape)
    items = cfg["item_count"]
    indexed = hasattr(m.lib, "tlsan_eval_topk_lists")          # (the parent's library has none)
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    cate = m.last_item_categories(db)
    out = lambda case, ms, **kw: print(json.dumps(dict(part=shape, case=case, ms=round(ms, 3), **kw)), flush=True)
    out("forward", timed(lambda: m.forward(db, is_test=True, want_u_t=True), n))
    out("recommend category", timed(lambda: m.recommend(db, K, category=cate), n))
    q = torch.randint(0, items, (B,), generator=torch.Generator(device="cpu").manual_seed(9)).numpy()
    for metric in ("cosine", "dot"):
        out("similar same_category " + metric, timed(lambda: m.similar_items(q, K, metric=metric, same_category=True), n))
        if shape == "even":
            out("similar plain " + metric, timed(lambda: m.similar_items(q, K, metric=metric), n))
    if not indexed:
        return
    t0 = time.perf_counter()
    idx = m.category_index()
    out("building the index", (time.perf_counter() - t0) * 1e3)
    lens = np.diff(idx.list_off.cpu().numpy())
    grid, idle, nsl, groups = idle_workgroups(cate.cpu().numpy(), lens)
    distinct = int(np.unique(cate.cpu().numpy()[cate.cpu().numpy() >= 0]).size)
    out("recommend category index", timed(lambda: m.recommend(db, K, category=cate, index=idx), n), workgroups=grid, idle=idle,
        slices=nsl, groups=groups, distinct=distinct, longest=int(lens.max()))
    for metric in ("cosine", "dot"):
        out("similar same_category index " + metric,
            timed(lambda: m.similar_items(q, K, metric=metric, same_category=True, index=idx), n))
    if shape == "even":
        one = m.item_scope(categories=[3])
        out("within one category (%d items)" % one.count, timed(lambda: m.recommend(db, K, within=one), n))


def lines_of(path, key):
    out = []
    with open(path, errors="replace") as f:
        for line in f:
            if line.startswith("{") and key in line:
                out.append(json.loads(line))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["even", "small", "skewed"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--lists", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "catidx"))
    a = ap.parse_args()
    if a.part:
        return part(a.part, a.iters)
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    steps = []
    for r in range(a.rounds if a.lists else 0):
        steps += [("even_%s_%d" % (side, r), me + ["--part", "even"], env, 300, ROOT) for side, env in sides]
    if a.lists:
        steps += [("small_this", me + ["--part", "small"], {}, 200, ROOT), ("skewed_this", me + ["--part", "skewed"], {}, 300, ROOT)]
    for r in range(a.rounds if a.bench else 0):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    print("B = Q = %d, K = %d; ms: median (min max of %d processes)" % (B, K, a.rounds))
    for side, _ in sides if a.lists else []:
        rows = {}
        for r in range(a.rounds):
            for row in lines_of(log_path(a.out, "even_%s_%d" % (side, r)), '"part"'):
                rows.setdefault(row["case"], []).append(row["ms"])
        for case, v in rows.items():
            v = sorted(v)
            print("even %-6s %-44s %10.3f   (%.3f %.3f)" % (side, case, v[len(v) // 2], v[0], v[-1]))
    for name in ("small_this", "skewed_this") if a.lists else ():
        for row in lines_of(log_path(a.out, name), '"part"'):
            extra = {k: v for k, v in row.items() if k not in ("part", "case", "ms")}
            print("%-11s %-44s %10.3f   %s" % (name, row["case"], row["ms"], json.dumps(extra) if extra else ""))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

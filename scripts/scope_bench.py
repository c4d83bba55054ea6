#!/usr/bin/env python3
"""Cost of the scoped lists (recommend's within= / category=, similar_items' same_category=) at d = 128, B = Q = 4096,
K = 10 over 5 M items in 200 categories (0.5 % of the items each), and what the item-mapping hook of topk_scan costs the
unscoped similar-items lists: this build against the parent commit's library in the same run.

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    recommend            plain, within = 100 % / 10 % / 1 % / 0.1 % of the items, category alone   (this build)
    similar_scoped       similar_items with same_category                                          (this build)
    similar_this_<r>     similar_items, plain, this build   } --rounds of them, interleaved
    similar_parent_<r>   similar_items, plain, --parent_lib }
    bench_this_<r>, bench_parent_<r>   bench.py's fp32 leg (ms_per_step_p50), interleaved -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one
as ab_run/<commit>.so); without it the parent's steps are left out.  Times are host clocks around a synchronised loop;
recommend's include the forward that produces u_t (printed beside them).

    python scripts/scope_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--items 5000000] [--out measure_out/scope]
    python scripts/scope_bench.py --part recommend|similar_plain|similar_scoped [--items N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, K, CATES = 4096, 10, 200
SHARES = (1.0, 0.1, 0.01, 0.001)


def timed(fn, n):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def big_model(items):
    from tlsan_amd import synth
    from tlsan_amd.model import Model
    cfg = synth.make_config("electronics", item_count=items, cate_count=CATES)
    return cfg, Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", init="device")


def part_recommend(items, n):
    import numpy as np
    from tlsan_amd import synth
    cfg, m = big_model(items)
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    rows = [("forward", timed(lambda: m.forward(db, is_test=True, want_u_t=True), n))]
    rows.append(("plain", timed(lambda: m.recommend(db, K), n)))
    rng = np.random.default_rng(5)
    for share in SHARES:
        ids = np.arange(items) if share == 1.0 else np.sort(rng.choice(items, int(items * share), replace=False))
        scope = m.item_scope(items=ids)
        rows.append(("within %g %% (%d items)" % (100 * share, scope.count), timed(lambda: m.recommend(db, K, within=scope), n)))
    cate = m.last_item_categories(db)
    rows.append(("category alone", timed(lambda: m.recommend(db, K, category=cate), n)))
    one = m.item_scope(categories=[3])
    rows.append(("within one category (%d items)" % one.count, timed(lambda: m.recommend(db, K, within=one), n)))
    for name, ms in rows:
        print(json.dumps(dict(part="recommend", case=name, ms=round(ms, 3))), flush=True)


def part_similar(items, n, scoped):
    import torch
    _, m = big_model(items)
    q = torch.randint(0, items, (B,), generator=torch.Generator(device="cpu").manual_seed(9)).numpy()
    for metric in ("cosine", "dot"):
        kw = dict(same_category=True) if scoped else {}
        ms = timed(lambda: m.similar_items(q, K, metric=metric, **kw), n)
        print(json.dumps(dict(part="similar_scoped" if scoped else "similar_plain", case=metric, ms=round(ms, 3))), flush=True)


def lines_of(path, key):
    out = []
    with open(path, errors="replace") as f:
        for line in f:
            if line.startswith("{") and key in line:
                out.append(json.loads(line))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["recommend", "similar_plain", "similar_scoped"])
    ap.add_argument("--items", type=int, default=5000000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "scope"))
    a = ap.parse_args()
    if a.part == "recommend":
        return part_recommend(a.items, a.iters)
    if a.part:
        return part_similar(a.items, a.iters, a.part == "similar_scoped")
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--items", a.items, "--iters", a.iters]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    steps = [("recommend", me + ["--part", "recommend"], {}, 420, ROOT), ("similar_scoped", me + ["--part", "similar_scoped"], {}, 300, ROOT)]
    for r in range(a.rounds):
        steps += [("similar_%s_%d" % (side, r), me + ["--part", "similar_plain"], env, 300, ROOT) for side, env in sides]
    for r in range(a.rounds):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    print("%-44s %10s" % ("recommend, B = %d, K = %d, %d items" % (B, K, a.items), "ms"))
    rec = lines_of(log_path(a.out, "recommend"), '"part"')
    for row in rec:
        print("%-44s %10.3f" % (row["case"], row["ms"]))
    t = {row["case"].split(" (")[0]: row["ms"] for row in rec}
    below = [s for s in SHARES if t["within %g %%" % (100 * s)] < t["plain"]]
    print("the scoped scan beats a plain scan (the cost of scanning everything and filtering afterwards) from a share of "
          "%s %% downwards" % ("%g" % (100 * max(below)) if below else "none of the measured"))
    for row in lines_of(log_path(a.out, "similar_scoped"), '"part"'):
        print("%-44s %10.3f" % ("similar_items same_category, " + row["case"], row["ms"]))
    for side, _ in sides:
        for metric in ("cosine", "dot"):
            v = sorted(row["ms"] for r in range(a.rounds) for row in lines_of(log_path(a.out, "similar_%s_%d" % (side, r)), '"part"')
                       if row["case"] == metric)
            print("%-44s %10.3f   (min %.3f max %.3f of %d)" % ("similar_items plain, %s, %s" % (metric, side), v[len(v) // 2],
                                                               v[0], v[-1], len(v)))
    for side, _ in sides:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-44s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

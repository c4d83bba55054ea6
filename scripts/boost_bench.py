#!/usr/bin/env python3
"""Cost of the boosted lists (recommend's boost= / boost_weight=) at B = 4096, K = 10, d = 128: every boosted call against the
unboosted call of the SAME entry point, in the same process, interleaved --

    scoped       tlsan_eval_topk_scoped with sub == NULL (the whole table, gather form) against tlsan_eval_topk_scoped_boost,
                 without and with row weights
    lists        tlsan_eval_topk_lists on a CategoryIndex (each row asks for the category of its last item) against
                 tlsan_eval_topk_lists_boost, without and with row weights
    recommend    plain recommend(), whose full scan may take the dense-matrix form, against recommend(boost=): what a caller
                 who adds boost= to a plain call sees (both include the forward that produces u_t)

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    synth_this                       5 M items in 200 categories (synth.py)
    small_this                       bench.py's Electronics tables: 22 048 items
    bench_this_<r>, bench_parent_<r> bench.py's fp32 leg (ms_per_step_p50) -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one);
without it the parent's steps are left out.  Times are host clocks around a synchronised loop of --iters calls behind a
warm-up.  The boost is Gaussian at the scale of the scores' spread, the weights uniform in [0, 2).

    python scripts/boost_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/boost]
    python scripts/boost_bench.py --part synth|small"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, K = 4096, 10
CASES = ("recommend", "recommend_boost", "scoped", "scoped_boost", "scoped_boost_w", "lists", "lists_boost", "lists_boost_w")


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


def part(shape, n, rounds):
    import torch
    from tlsan_amd import synth
    from tlsan_amd.model import index_categories, lists_topk, scoped_topk
    cfg, m = model_of(shape)
    I = cfg["item_count"]
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    out = lambda case, **kw: print(json.dumps(dict(part=shape, case=case, **kw)), flush=True)
    _, _, ut, _ = m.forward(db, is_test=True, want_u_t=True)
    st, cp, none, ws = m._stream(), m.cparams, (None, None), m._topk_workspace
    plain = m.recommend(db, K)
    gen = torch.Generator(device=m.device).manual_seed(5)
    spread = float(plain[1].float().std())
    values = torch.randn(I, device=m.device, generator=gen) * spread
    weight = torch.rand(B, device=m.device, generator=gen) * 2
    held = m.item_boost(values)
    index = m.category_index()
    lists = index.local(1, 0, I)
    rows = index_categories(m.last_item_categories(db), B, cfg["cate_count"], m.device)
    asked = lists[0].long()[rows[:, 0].clamp(min=0).long() + 1] - lists[0].long()[rows[:, 0].clamp(min=0).long()]
    out("shape", items=I, score_spread=round(spread, 5), max_list=lists[2], mean_asked_list=round(float(asked.float().mean()), 1))
    # what the boost does to the lists, and that the zero boost changes nothing (ids and score bits)
    boosted = m.recommend(db, K, boost=held)
    zero = m.recommend(db, K, boost=torch.zeros(I, device=m.device))
    out("effect", rows_changed=int((boosted[0] != plain[0]).any(1).sum()),
        zero_equal=bool(torch.equal(zero[0], plain[0]) and torch.equal(zero[1].view(torch.int32), plain[1].view(torch.int32))))
    b, bw = (held.values, None), (held.values, weight)
    calls = dict(
        recommend=lambda: m.recommend(db, K),
        recommend_boost=lambda: m.recommend(db, K, boost=held),
        scoped=lambda: scoped_topk(m.lib, m.dims, cp, ut, B, K, none, None, None, 1, 0, ws, st),
        scoped_boost=lambda: scoped_topk(m.lib, m.dims, cp, ut, B, K, none, None, None, 1, 0, ws, st, boost=b),
        scoped_boost_w=lambda: scoped_topk(m.lib, m.dims, cp, ut, B, K, none, None, None, 1, 0, ws, st, boost=bw),
        lists=lambda: lists_topk(m.lib, m.dims, cp, ut, B, K, none, lists, rows, 1, 0, ws, st),
        lists_boost=lambda: lists_topk(m.lib, m.dims, cp, ut, B, K, none, lists, rows, 1, 0, ws, st, boost=b),
        lists_boost_w=lambda: lists_topk(m.lib, m.dims, cp, ut, B, K, none, lists, rows, 1, 0, ws, st, boost=bw))
    for r in range(rounds):                                     # interleaved: every case once per round
        for case in CASES:
            out(case, round=r, ms=round(timed(calls[case], n), 4))


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
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--lists", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "boost"))
    a = ap.parse_args()
    if a.part:
        return part(a.part, a.iters, a.rounds)
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters, "--rounds", a.rounds]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    steps = []
    if a.lists:
        steps += [("synth_this", me + ["--part", "synth"], {}, 600, ROOT), ("small_this", me + ["--part", "small", "--iters", 10 * a.iters], {}, 300, ROOT)]
    for r in range(a.rounds if a.bench else 0):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: "%9.4f (%.4f %.4f)" % (med(v), min(v), max(v))
    print("B = %d, K = %d; ms: median (min max) of %d interleaved rounds" % (B, K, a.rounds))
    for name in ("synth_this", "small_this") if a.lists else ():
        rows = lines_of(log_path(a.out, name), '"part"')
        for s in (r for r in rows if r["case"] in ("shape", "effect")):
            print("%-11s %s" % (name, json.dumps({k: v for k, v in s.items() if k not in ("part", "case")})))
        ms = lambda case: [r["ms"] for r in rows if r["case"] == case]
        for case in CASES:
            twin = case.split("_boost")[0]
            print("%-11s %-16s %s   x%.4f of %s" % (name, case, fmt(ms(case)), med(ms(case)) / med(ms(twin)), twin))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

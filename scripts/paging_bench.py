#!/usr/bin/env python3
"""Cost of the list cursors (recommend's and audience's after=) at B = 4096, K = 10, d = 128, on boost_bench.py's tables: every
call behind a cursor against its twin without one, in the same process, interleaved --

    scoped         tlsan_eval_topk_scoped with sub == NULL (the whole table, gather form) against tlsan_eval_topk_scoped_after
                   at START (page 1), and pages 2, 10 and 100 of the same ranking (cursors behind entries 10, 90 and 990)
    boost          tlsan_eval_topk_scoped_boost against tlsan_eval_topk_scoped_after with the boost, at START
    lists          tlsan_eval_topk_lists on a CategoryIndex (each row asks for the category of its last item) against
                   tlsan_eval_topk_lists_after at START, and page 2
    audience       (--part audience) tlsan_dense_topk over N = 200 000 rows for Q = 256 queries, K = 256, against
                   tlsan_dense_topk_after at START; and audience_deep's chain of 16 pages (n = 4096) against 16 calls of K = 256

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    synth_this                       5 M items in 200 categories (synth.py)
    small_this                       bench.py's Electronics tables: 22 048 items
    audience_this                    the dense call
    bench_this_<r>, bench_parent_<r> bench.py's fp32 leg (ms_per_step_p50) -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one);
without it the parent's steps are left out.  Times are host clocks around a synchronised loop of --iters calls behind a
warm-up.  The cursors of the deep pages come from recommend_deep, so every timed page is a real page of the ranking.

    python scripts/paging_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/paging]
    python scripts/paging_bench.py --part synth|small|audience"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, K = 4096, 10
CASES = ("scoped", "scoped_after_start", "scoped_after_page2", "scoped_after_page10", "scoped_after_page100",
         "boost", "boost_after_start", "lists", "lists_after_start", "lists_after_page2")
AUD_N, AUD_Q, AUD_K, AUD_D, AUD_PAGES = 200000, 256, 256, 128, 16
AUD_CASES = ("dense", "dense_after_start", "dense_x16", "dense_deep16")
TWIN = dict(scoped_after_start="scoped", scoped_after_page2="scoped_after_start", scoped_after_page10="scoped_after_start",
            scoped_after_page100="scoped_after_start", boost_after_start="boost", lists_after_start="lists",
            lists_after_page2="lists_after_start", dense_after_start="dense", dense_deep16="dense_x16")


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
    from tlsan_amd.model import ListCursor, index_categories, lists_topk, scoped_topk
    cfg, m = model_of(shape)
    I = cfg["item_count"]
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    out = lambda case, **kw: print(json.dumps(dict(part=shape, case=case, **kw)), flush=True)
    _, _, ut, _ = m.forward(db, is_test=True, want_u_t=True)
    st, cp, none, ws = m._stream(), m.cparams, (None, None), m._topk_workspace
    deep = m.recommend_deep(db, 100 * K)                           # the ranking to depth 1000: the pages' cursors
    cur = lambda page: ListCursor.of(deep[0][:, :(page - 1) * K], deep[1][:, :(page - 1) * K]) if page > 1 else ListCursor.start(B, m.device)
    gen = torch.Generator(device=m.device).manual_seed(5)
    values = torch.randn(I, device=m.device, generator=gen) * float(deep[1][:, :K].float().std())
    boost = (m.item_boost(values).values, None)
    index = m.category_index()
    lists = index.local(1, 0, I)
    rows = index_categories(m.last_item_categories(db), B, cfg["cate_count"], m.device)
    sc = lambda **kw: scoped_topk(m.lib, m.dims, cp, ut, B, K, none, None, None, 1, 0, ws, st, **kw)
    ls = lambda **kw: lists_topk(m.lib, m.dims, cp, ut, B, K, none, lists, rows, 1, 0, ws, st, **kw)
    lp1 = ls()
    same = lambda a, b: bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    # START is the twin, and page 100 is the ranking's entries 990 .. 999 (ids and score bits)
    out("check", items=I, start_equal=same(sc(after=cur(1)), sc()), boost_start_equal=same(sc(boost=boost, after=cur(1)), sc(boost=boost)),
        lists_start_equal=same(ls(after=cur(1)), lp1),
        page100_equal=same(sc(after=cur(100)), (deep[0][:, 99 * K:], deep[1][:, 99 * K:])))
    c1, c2, c10, c100, lc2 = cur(1), cur(2), cur(10), cur(100), ListCursor.of(*lp1)
    calls = dict(
        scoped=lambda: sc(), scoped_after_start=lambda: sc(after=c1), scoped_after_page2=lambda: sc(after=c2),
        scoped_after_page10=lambda: sc(after=c10), scoped_after_page100=lambda: sc(after=c100),
        boost=lambda: sc(boost=boost), boost_after_start=lambda: sc(boost=boost, after=c1),
        lists=lambda: ls(), lists_after_start=lambda: ls(after=c1), lists_after_page2=lambda: ls(after=lc2))
    for r in range(rounds):                                     # interleaved: every case once per round
        for case in CASES:
            out(case, round=r, ms=round(timed(calls[case], n), 4))


def audience_part(n, rounds):
    import torch
    from tlsan_amd import _lib as L
    from tlsan_amd.model import ListCursor, deep_pages, dense_topk
    lib, dev = L.load(), torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(AUD_N)
    x = torch.randn(AUD_N, AUD_D, device=dev, generator=g)
    q = torch.randn(AUD_Q, AUD_D, device=dev, generator=g)
    scale, bias = torch.full((AUD_Q,), 0.75, device=dev), torch.randn(AUD_Q, device=dev, generator=g)
    st, held = torch.cuda.current_stream(dev).cuda_stream, {}

    def workspace(nbytes):
        if held.get("ws") is None or held["ws"].numel() < nbytes:
            held["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return held["ws"]
    out = lambda case, **kw: print(json.dumps(dict(part="audience", case=case, **kw)), flush=True)
    call = lambda k, after=None: dense_topk(lib, q, x, scale, bias, (None, None), 0, k, workspace, st, after=after)
    start = ListCursor.start(AUD_Q, dev)
    deep = deep_pages(call, AUD_PAGES * AUD_K, AUD_K)
    flat = ((q @ x.T) * scale[:, None] + bias[:, None]).topk(AUD_PAGES * AUD_K, dim=1).indices    # the same rows, to the last bits' ties
    out("check", rows=AUD_N, queries=AUD_Q, start_equal=bool(torch.equal(call(AUD_K, start)[0], call(AUD_K)[0])),
        deep_rows_agree=round(float((deep[0].long().sort(1).values == flat.sort(1).values).float().mean()), 5))
    calls = dict(dense=lambda: call(AUD_K), dense_after_start=lambda: call(AUD_K, start),
                 dense_x16=lambda: [call(AUD_K) for _ in range(AUD_PAGES)], dense_deep16=lambda: deep_pages(call, AUD_PAGES * AUD_K, AUD_K))
    for r in range(rounds):
        for case in AUD_CASES:
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
    ap.add_argument("--part", choices=["synth", "small", "audience"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--lists", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "paging"))
    a = ap.parse_args()
    if a.part:
        return audience_part(a.iters, a.rounds) if a.part == "audience" else part(a.part, a.iters, a.rounds)
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters, "--rounds", a.rounds]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    steps = []
    if a.lists:
        steps += [("synth_this", me + ["--part", "synth"], {}, 600, ROOT), ("small_this", me + ["--part", "small", "--iters", 10 * a.iters], {}, 300, ROOT),
                  ("audience_this", me + ["--part", "audience"], {}, 300, ROOT)]
    for r in range(a.rounds if a.bench else 0):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: "%9.4f (%.4f %.4f)" % (med(v), min(v), max(v))
    print("B = %d, K = %d; ms: median (min max) of %d interleaved rounds" % (B, K, a.rounds))
    for name, cases in (("synth_this", CASES), ("small_this", CASES), ("audience_this", AUD_CASES)) if a.lists else ():
        rows = lines_of(log_path(a.out, name), '"part"')
        for s in (r for r in rows if r["case"] == "check"):
            print("%-13s %s" % (name, json.dumps({k: v for k, v in s.items() if k not in ("part", "case")})))
        ms = lambda case: [r["ms"] for r in rows if r["case"] == case]
        for case in cases:
            twin = TWIN.get(case)
            print("%-13s %-22s %s%s" % (name, case, fmt(ms(case)), "   x%.4f of %s" % (med(ms(case)) / med(ms(twin)), twin) if twin else ""))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

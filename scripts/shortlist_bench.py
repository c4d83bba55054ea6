#!/usr/bin/env python3
"""Cost and certified share of the bf16 shortlist index (recommend's index=<ShortlistIndex>) at B = 4096, K = 10 against the
exact recommend() -- the fp32 scan of every item, the parent commit's path, untouched -- timed in the same process, interleaved.

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    synth_this                       5 M items in 200 categories (synth.py), d = 128: the build, then for N in 64, 128, 256 the
                                     certified share and three rounds of [exact recommend, the two-stage call, stage 1 alone,
                                     re-score + select alone, the fallback's sub-batch alone]; then the cells of "when not to
                                     use it": one item of 50 times the norm, and K = 50 of N = 64; then the same table with
                                     Gaussian item vectors (scores spaced, not crowded): share, exact and two-stage times
    small_this                       bench.py's Electronics tables: 63 001 items, the same sweep
    bench_this_<r>, bench_parent_<r> bench.py's fp32 leg (ms_per_step_p50) -- that path is untouched

and prints the table.  --parent_lib: the parent commit's libtlsan_hip.so (scripts/mkvariants.sh rev:<commit> builds one);
without it the parent's steps are left out.  Times are host clocks around a synchronised loop of --iters calls behind a
warm-up; recommend's include the forward that produces u_t, the stages' do not.  A library built with another
SHORTLIST_T (csrc/tlsan_shortlist.h), loaded through TLSAN_LIB_PATH, gives the times of another number of row tiles per workgroup.

    python scripts/shortlist_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/shortlist]
    python scripts/shortlist_bench.py --part synth|small"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, K = 4096, 10
NS = (64, 128, 256)


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


def part(shape, n, rounds, ns):
    import torch
    from tlsan_amd import shortlist as S
    from tlsan_amd.model import eval_topk, score_candidates
    cfg, m = model_of(shape)
    from tlsan_amd import synth
    db = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    out = lambda case, **kw: print(json.dumps(dict(part=shape, case=case, **kw)), flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = m.shortlist_index()
    torch.cuda.synchronize()
    out("build", ms=round((time.perf_counter() - t0) * 1e3, 2), wmax=float(index.wmax.item()))
    _, _, ut, _ = m.forward(db, is_test=True, want_u_t=True)
    st, cp, none = m._stream(), m.cparams, (None, None)
    exact = m.recommend(db, K)

    def share(k, N, idx):
        got = m.recommend(db, k, index=idx, shortlist=N)
        want = exact if k == K else m.recommend(db, k)
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)))
        return round(float(idx.certified.float().mean()), 4), same

    for N in ns:
        cert, same = share(K, N, index)
        out("share", N=N, K=K, certified=cert, equal_to_exact=same)
        sid, approx = S.stage1(m.lib, index, ut, B, N, none, cp.scale, cp.item_b, cp.ld_itemb or 1, 1, 0, m._topk_workspace, st)
        sc = score_candidates(m.lib, m.dims, cp, ut, sid, 1, 0, st)
        rows = (~index.certified).nonzero().reshape(-1)
        sub = ut[rows].contiguous() if rows.numel() else None
        for r in range(rounds):                                 # the exact scan and the two-stage call, interleaved
            out("exact", N=N, round=r, ms=round(timed(lambda: m.recommend(db, K), n), 3))
            out("total", N=N, round=r, ms=round(timed(lambda: m.recommend(db, K, index=index, shortlist=N), n), 3))
            out("stage1", N=N, round=r, ms=round(timed(lambda: S.stage1(m.lib, index, ut, B, N, none, cp.scale, cp.item_b, cp.ld_itemb or 1,
                                                                      1, 0, m._topk_workspace, st), n), 3))
            out("stage2", N=N, round=r, ms=round(timed(lambda: S.select(m.lib, index, sid, score_candidates(m.lib, m.dims, cp, ut, sid, 1, 0, st),
                                                                      approx, ut, cp.scale, K, st), n), 3))
            fb = 0.0 if sub is None else timed(lambda: eval_topk(m.lib, m.dims, cp, sub, int(rows.numel()), K, none, 1, 0, m._topk_workspace, st), n)
            out("fallback", N=N, round=r, rows=int(rows.numel()), ms=round(fb, 3))
        del sid, approx, sc
    # when not to use it: K large against N; one item of a huge norm (the bound is wmax)
    cert, same = share(50, 64, index)
    out("share", N=64, K=50, certified=cert, equal_to_exact=same)
    row = m.item_emb[7].clone()
    m.item_emb[7] = row * 50.0
    big = m.shortlist_index()
    exact = m.recommend(db, K)
    cert, same = share(K, 64, big)
    out("share_huge_norm", N=64, K=K, certified=cert, equal_to_exact=same, wmax=float(big.wmax.item()))
    m.item_emb[7] = row
    if shape == "synth":
        # the same table with Gaussian item vectors of the category vectors' spread: scores spaced like a trained table's top,
        # where the untrained synthetic rows (tiny item vectors: a category's items score alike) are crowded
        m.item_emb.normal_(0.0, float(m.cate_emb.float().std()))
        gauss = m.shortlist_index()
        exact = m.recommend(db, K)
        for N in ns:
            cert, same = share(K, N, gauss)
            out("share_gauss", N=N, K=K, certified=cert, equal_to_exact=same, wmax=float(gauss.wmax.item()))
            for r in range(rounds):
                out("exact_gauss", N=N, round=r, ms=round(timed(lambda: m.recommend(db, K), n), 3))
                out("total_gauss", N=N, round=r, ms=round(timed(lambda: m.recommend(db, K, index=gauss, shortlist=N), n), 3))


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
    ap.add_argument("--n", default=",".join(str(x) for x in NS), help="the shortlist lengths")
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--lists", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "shortlist"))
    a = ap.parse_args()
    if a.part:
        return part(a.part, a.iters, a.rounds, [int(x) for x in a.n.split(",")])
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters, "--rounds", a.rounds, "--n", a.n]
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
    fmt = lambda v: "%9.3f (%.3f %.3f)" % (med(v), min(v), max(v))
    print("B = %d, K = %d; ms: median (min max) of %d interleaved rounds" % (B, K, a.rounds))
    for name in ("synth_this", "small_this") if a.lists else ():
        rows = lines_of(log_path(a.out, name), '"part"')
        for b in (r for r in rows if r["case"] == "build"):
            print("%-11s build %.2f ms, wmax %.4f" % (name, b["ms"], b["wmax"]))
        for s in (r for r in rows if r["case"].startswith("share")):
            print("%-11s %-16s N %3d K %2d  certified %.4f  equal to the exact lists: %s" % (name, s["case"], s["N"], s["K"], s["certified"], s["equal_to_exact"]))
        for N in sorted(set(r["N"] for r in rows if r["case"] == "total")):
            ms = lambda case: [r["ms"] for r in rows if r["case"] == case and r["N"] == N]
            print("%-11s N %3d  exact %s  two-stage %s  x%.2f | stage 1 %s  re-score + select %s  fallback %s (%d rows)"
                  % (name, N, fmt(ms("exact")), fmt(ms("total")), med(ms("exact")) / med(ms("total")), fmt(ms("stage1")), fmt(ms("stage2")),
                     fmt(ms("fallback")), [r["rows"] for r in rows if r["case"] == "fallback" and r["N"] == N][0]))
        for N in sorted(set(r["N"] for r in rows if r["case"] == "total_gauss")):
            ms = lambda case: [r["ms"] for r in rows if r["case"] == case and r["N"] == N]
            print("%-11s Gaussian items  N %3d  exact %s  two-stage %s  x%.2f" % (name, N, fmt(ms("exact_gauss")), fmt(ms("total_gauss")),
                                                                                 med(ms("exact_gauss")) / med(ms("total_gauss"))))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

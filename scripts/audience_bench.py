#!/usr/bin/env python3
"""Cost of the dense top-K call behind the audience lists (tlsan_dense_topk) alone, on random matrices -- the call reads
no table -- at d = 128, K = 10, N = 200 k and 10 M rows, Q = 1, 16, 256 and 4096 queries, against what a caller could do
before it existed, timed in the same process, interleaved: a chunked `q @ x.T` (scaled, biased) with torch.topk per chunk
and one more over the chunks' candidates, the chunks sized so that a [Q, chunk] fp32 score block stays within 1 GiB.

Without --part this is a list of steps for scripts/steps.py (one program after another, each under its own time limit,
nothing more after the first that fails; logs under --out):

    rows_200k, rows_10m              the sweep over Q at that N: --rounds rounds of [the call, the workaround] per Q
    bench_this_<r>, bench_parent_<r> bench.py's fp32 leg (ms_per_step_p50) -- the training step is untouched

and prints the table: median (min max) of the rounds, and the bytes the scan must move, ceil(Q / 16) * N * d * 4 (every
tile of 16 queries streams the matrix once), over its time.  --parent_lib: the parent commit's libtlsan_hip.so
(scripts/mkvariants.sh rev:<commit> builds one); without it the parent's steps are left out.  Times are host clocks
around a synchronised loop of --iters calls behind a warm-up.

    python scripts/audience_bench.py [--parent_lib ab_run/<commit>.so] [--rounds 3] [--out measure_out/audience]
    python scripts/audience_bench.py --part 200000|10000000"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

D, K = 128, 10
QS = (1, 16, 256, 4096)
NS = (200000, 10000000)
BLOCK_BYTES = 1 << 30      # the workaround's [Q, chunk] score block


def timed(fn, n):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def workaround(q, x, scale, bias, k):
    """The K best rows per query by materialised score blocks: chunked q @ x.T, torch.topk per chunk and over the chunks."""
    import torch
    Q, N = q.shape[0], x.shape[0]
    chunk = max(k, min(N, BLOCK_BYTES // (4 * Q)))
    vals, idx = [], []
    for n0 in range(0, N, chunk):
        s = (q @ x[n0:n0 + chunk].T) * scale[:, None] + bias[:, None]
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        vals.append(v)
        idx.append(i + n0)
    v, j = torch.topk(torch.cat(vals, 1), k, dim=1)
    return torch.gather(torch.cat(idx, 1), 1, j), v


def part(N, iters, rounds):
    import torch
    from tlsan_amd import _lib as L
    from tlsan_amd.model import dense_topk
    lib, dev = L.load(), torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(N)
    x = torch.randn(N, D, device=dev, generator=g)
    st = torch.cuda.current_stream(dev).cuda_stream
    held = {}

    def workspace(nbytes):
        if held.get("ws") is None or held["ws"].numel() < nbytes:
            held["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return held["ws"]
    out = lambda case, **kw: print(json.dumps(dict(part=N, case=case, **kw)), flush=True)
    for Q in QS:
        q = torch.randn(Q, D, device=dev, generator=g)
        scale = torch.full((Q,), 0.75, device=dev)
        bias = torch.randn(Q, device=dev, generator=g)
        call = lambda: dense_topk(lib, q, x, scale, bias, (None, None), 0, K, workspace, st)
        other = lambda: workaround(q, x, scale, bias, K)
        a, b = call()[0], other()[0]                              # the same rows but for scores that differ in the last bits
        agree = float((a.long().sort(1).values == b.sort(1).values).float().mean().item())
        n = iters if Q * N <= 4096 * 200000 else max(1, iters // 3)
        for r in range(rounds):                                   # the call and the workaround, interleaved
            out("call", Q=Q, round=r, ms=round(timed(call, n), 4))
            out("torch", Q=Q, round=r, ms=round(timed(other, n), 4))
        out("agree", Q=Q, rows_agree=round(agree, 5))


def lines_of(path, key):
    rows = []
    with open(path, errors="replace") as f:
        for line in f:
            if line.startswith("{") and key in line:
                rows.append(json.loads(line))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", type=int, choices=list(NS))
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", type=int, default=1, help="0: leave bench.py's steps out")
    ap.add_argument("--lists", type=int, default=1, help="0: bench.py's steps only")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--out", default=os.path.join("measure_out", "audience"))
    a = ap.parse_args()
    if a.part:
        return part(a.part, a.iters, a.rounds)
    from steps import log_path, run_steps
    me = [sys.executable, os.path.abspath(__file__), "--iters", a.iters, "--rounds", a.rounds]
    bench = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
    sides = [("this", {})] + ([("parent", {"TLSAN_LIB_PATH": os.path.abspath(a.parent_lib)})] if a.parent_lib else [])
    names = {200000: "rows_200k", 10000000: "rows_10m"}
    steps = [(names[N], me + ["--part", N], {}, 420, ROOT) for N in NS] if a.lists else []
    for r in range(a.rounds if a.bench else 0):
        steps += [("bench_%s_%d" % (side, r), bench, env, 300, ROOT) for side, env in sides]
    rc = run_steps(steps, a.out)
    if rc:
        return rc
    med = lambda v: sorted(v)[len(v) // 2]
    print("d = %d, K = %d; ms: median (min max) of %d interleaved rounds; GB/s: ceil(Q / 16) * N * d * 4 bytes over the call's median"
          % (D, K, a.rounds))
    for N in NS if a.lists else ():
        rows = lines_of(log_path(a.out, names[N]), '"part"')
        for Q in QS:
            c = [r["ms"] for r in rows if r["case"] == "call" and r["Q"] == Q]
            t = [r["ms"] for r in rows if r["case"] == "torch" and r["Q"] == Q]
            agree = [r["rows_agree"] for r in rows if r["case"] == "agree" and r["Q"] == Q][0]
            moved = -(-Q // 16) * N * D * 4
            print("N %9d  Q %5d  tlsan_dense_topk %10.4f (%.4f %.4f)  %8.1f GB/s   matmul + topk %10.4f (%.4f %.4f)  x%.2f  rows agree %.5f"
                  % (N, Q, med(c), min(c), max(c), moved / med(c) / 1e6, med(t), min(t), max(t), med(t) / med(c), agree))
    for side, _ in sides if a.bench else []:
        v = sorted(lines_of(log_path(a.out, "bench_%s_%d" % (side, r)), '"metric"')[-1]["ms_per_step_p50"] for r in range(a.rounds))
        print("%-56s %10.4f   (min %.4f max %.4f of %d)" % ("bench.py ms_per_step_p50, " + side, v[len(v) // 2], v[0], v[-1], len(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

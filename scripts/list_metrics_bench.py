#!/usr/bin/env python3
"""Cost of measuring lists (tlsan_list_metrics, k_list_metrics) beside the kernel that does the same K x K x d products
with a dependent selection step between them, tlsan_rerank at N = K, theta = 0.5 and no cap: B = 4096 lists of an
electronics-scale synthetic table (I = 22 048, 673 categories), K in {10, 100, 256}, d in {64, 128, 256}.  Both are timed
in one process on the same staged inputs (Model.recommend(k = K)'s lists, their vectors, inverse norms and categories,
staged once outside the timed window), alternating call by call; a time is device events around one call, and p10 / p50 /
p90 are over all timed calls of every round.  --parent_lib: the library tlsan_rerank is called through (the parent
commit's build; default: this build's, whose re-ranking unit is the parent's unchanged).

    python scripts/list_metrics_bench.py [--out FILE]               every d as a step of scripts/steps.py, then the report
    python scripts/list_metrics_bench.py --measure D --json FILE    one d (a step of the above)
    python scripts/list_metrics_bench.py --tradeoff [--out FILE]    the quality table of the diversity settings (driver runs)
The two reports (measure_out/list_metrics/times.md and tradeoff.md by default) make up profiles/list_metrics.md."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
B, THETA, CAP, KS_, ROUNDS = 4096, 0.5, 0, (10, 100, 256), 3


def timed(fns, n):
    """n calls of each of fns, alternating call by call, after three warm-up calls each -> a list of times (ms) per fn"""
    import torch
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(n):
        for t, fn in zip(times, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return times


def pcts(t):
    t = sorted(t)
    at = lambda q: t[min(len(t) - 1, int(round(q * (len(t) - 1))))]
    return dict(p10=at(0.1), p50=at(0.5), p90=at(0.9))


def measure(d, path, n, parent_lib):
    import torch
    from tlsan_amd import _lib as L
    from tlsan_amd import model as M
    from tlsan_amd import synth
    cfg = synth.make_config("electronics", hidden_units=d, itemid_embedding_size=d // 2, userid_embedding_size=d // 2,
                            cateid_embedding_size=d // 2)
    m = M.Model(cfg, synth.item_cate_list(cfg), init="device")
    rr = m.lib
    if parent_lib:
        rr = C.CDLL(os.path.abspath(parent_lib))
        rr.tlsan_rerank.argtypes, rr.tlsan_rerank.restype = m.lib.tlsan_rerank.argtypes, C.c_int
        rr.tlsan_last_error.restype = C.c_char_p
        assert rr.tlsan_abi_version() == L.ABI_VERSION and not hasattr(rr, "tlsan_list_metrics")
    batch = synth.make_batches(cfg, 1, batch_size=B, test=True)[0]
    db = m.device_batch(batch, is_test=True)
    weight = torch.rand(cfg["item_count"], device=m.device)
    out = []
    for K in KS_:
        pid, psc = m.recommend(db, K, exclude="history")
        rows = min(B, M.rerank_chunk(K, d))
        pid, psc = pid[:rows].contiguous(), psc[:rows].contiguous()
        flat = pid.reshape(-1)
        vec, inv = M.item_vectors(m.lib, m.dims, m.cparams, flat, 1, 0, m._stream())
        g = flat.clamp(min=0).long()
        cate, w = m.item_cate[g], weight[g]
        expo = torch.zeros(cfg["item_count"], dtype=torch.int32, device=m.device)
        ids = torch.empty(rows, K, dtype=torch.int32, device=m.device)
        sc = torch.empty(rows, K, dtype=torch.float32, device=m.device)
        lab = db.i[:rows].to(torch.int32).contiguous()
        o32 = [torch.empty(rows, dtype=torch.int32, device=m.device) for _ in range(4)]      # n, n_cate, max_cate, hit_pos
        o64 = [torch.empty(rows, dtype=torch.float64, device=m.device) for _ in range(2)]    # pair_cos, weight_sum
        # the entry point alone, outputs allocated once like tlsan_rerank's (Model.list_metrics adds the ILD on top)
        listm = lambda: L.check(m.lib.tlsan_list_metrics(
            pid.data_ptr(), vec.data_ptr(), inv.data_ptr(), cate.data_ptr(), lab.data_ptr(), w.data_ptr(), rows, K, d,
            o32[0].data_ptr(), o64[0].data_ptr(), o32[1].data_ptr(), o32[2].data_ptr(), o32[3].data_ptr(), o64[1].data_ptr(),
            expo.data_ptr(), int(expo.shape[0]), m._stream()), "tlsan_list_metrics")
        rerank = lambda: M.rerank(rr, pid, psc, vec, inv, cate, K, THETA, CAP, ids, sc, m._stream())
        t_l, t_r = [], []
        for _ in range(ROUNDS):
            a, b = timed((listm, rerank), n)
            t_l += a
            t_r += b
        assert int((ids < 0).sum().item()) == 0 and int(o32[0].min().item()) == K      # every row ran its K steps
        out.append(dict(d=d, K=K, rows=rows, list_metrics_ms=pcts(t_l), rerank_ms=pcts(t_r), calls=len(t_l)))
        print(json.dumps(out[-1]), flush=True)
    with open(path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), parent_lib=bool(parent_lib), rows=out), f, indent=1)


def digest(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def report(out, log_dir, n, parent_lib):
    from steps import log_path, run_steps
    py = sys.executable
    steps = [("registers", [py, os.path.join(ROOT, "scripts", "kernel_registers.py"), "--all", "tlsan_listm"], None, 300, ROOT)]
    extra = ["--parent_lib", parent_lib] if parent_lib else []
    steps += [("d%d" % d, [py, os.path.abspath(__file__), "--measure", d, "--json", os.path.join(log_dir, "d%d.json" % d),
                           "--iters", n] + extra, None, 420, ROOT) for d in (64, 128, 256)]
    rc = run_steps(steps, log_dir)
    if rc:
        return rc
    csrc = os.path.join(ROOT, "tlsan_amd", "csrc")
    res = [json.load(open(os.path.join(log_dir, "d%d.json" % d))) for d in (64, 128, 256)]
    hipcc = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
    lines = ["## Registers (`scripts/kernel_registers.py --all tlsan_listm`; `k_list_metrics<D, threads>`, occupancy in waves per SIMD)", "",
             "```", open(log_path(log_dir, "registers")).read().strip(), "```", "",
             "## Times", "",
             "Made by `python scripts/list_metrics_bench.py` (steps of `scripts/steps.py`, one per d).  Build: `libtlsan_hip.so` sha256 `%s`,"
             % digest([os.path.join(ROOT, "tlsan_amd", "libtlsan_hip.so")]),
             "`tlsan_listm.h` + `tlsan_listm.hip` sha256 `%s`, %s; device %s.  `tlsan_rerank` through %s." % (
                 digest([os.path.join(csrc, "tlsan_listm.h"), os.path.join(csrc, "tlsan_listm.hip")]),
                 hipcc[0] if hipcc else "hipcc unknown", res[0]["device"],
                 "the parent commit's library (sha256 `%s`)" % digest([parent_lib]) if parent_lib else "this build"), "",
             "B = %d lists (`rows` of them: one chunk of the 256 MB staging rule) of an electronics-scale table (I = 22 048); `rerank`:"
             % B,
             "`tlsan_rerank` at N = K, theta = %.1f, no cap, on the same staged inputs.  Device events around one call, the two kernels" % THETA,
             "alternating call by call, %d rounds of %d calls each; ms, p10 / p50 / p90 over all calls." % (ROUNDS, n), "",
             "| d | K | rows | list_metrics p10 | p50 | p90 | rerank p10 | p50 | p90 | p50 ratio |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        for x in r["rows"]:
            a, b = x["list_metrics_ms"], x["rerank_ms"]
            lines.append("| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f |" % (
                x["d"], x["K"], x["rows"], a["p10"], a["p50"], a["p90"], b["p10"], b["p50"], b["p90"], a["p50"] / b["p50"]))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
    return 0


TRADEOFF_STEPS, TRADEOFF_K = 3000, 10


def tradeoff(out, log_dir):
    """The table the measurement exists for: the driver on the clothing fixture, TRADEOFF_STEPS steps from the same seeds
    (the same model every time), then --recommend_metrics over theta x per_category at K = 10 -- recorded, not asserted."""
    from steps import run_steps
    ds = os.path.join(ROOT, "tests", "golden", "packed_clothing.npz")
    grid = [(theta, m) for m in (0, 2) for theta in (0.0, 0.25, 0.5, 0.75)]
    name = lambda theta, m: "theta%03d_m%d" % (round(100 * theta), m)
    steps = [(name(theta, m), [sys.executable, "-m", "tlsan_amd.train", "--dataset", ds, "--model_dir", os.path.join(log_dir, name(theta, m)),
                               "--max_steps", TRADEOFF_STEPS, "--eval_freq", 1000, "--eval_topk", 0, "--quiet", "--recommend_k", TRADEOFF_K,
                               "--recommend_diversity", theta, "--recommend_per_category", m, "--recommend_metrics", 1],
              None, 300, ROOT) for theta, m in grid]
    rc = run_steps(steps, log_dir)
    if rc:
        return rc
    k = TRADEOFF_K
    cols = ["NDCG@%d" % k, "HR@%d" % k, "ILD@%d" % k, "categories@%d" % k, "max_per_category", "coverage@%d" % k, "gini@%d" % k,
            "novelty@%d" % k, "short_rows"]
    lines = ["## What the diversity settings buy and cost", "",
             "`python scripts/list_metrics_bench.py --tradeoff`: `python -m tlsan_amd.train` on `tests/golden/packed_clothing.npz`, %d steps"
             % TRADEOFF_STEPS,
             "from the same seeds for every row (the same model), then `--recommend_k %d --recommend_metrics 1` with the row's" % k,
             "`--recommend_diversity` (theta) and `--recommend_per_category`; exclude = history, the default pool.  Recorded, not asserted.", "",
             "| theta | per_category | " + " | ".join(cols) + " | rows |", "|---" * (len(cols) + 3) + "|"]
    for theta, m in grid:
        r = json.load(open(os.path.join(log_dir, name(theta, m), "recommend_top%d_metrics.json" % k)))
        lines.append("| %.2f | %d | " % (theta, m) + " | ".join(
            ("%d" % r[c]) if isinstance(r[c], int) else ("%.4f" % r[c]) for c in cols) + " | %d |" % r["rows"])
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", type=int, default=0, choices=[0, 64, 128, 256])
    ap.add_argument("--json", default=None)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--tradeoff", action="store_true", help="the quality table of the diversity settings instead of the times")
    ap.add_argument("--out", default=os.path.join(ROOT, "measure_out", "list_metrics", "times.md"))
    ap.add_argument("--log_dir", default=os.path.join(ROOT, "measure_out", "list_metrics"))
    a = ap.parse_args()
    if a.measure:
        measure(a.measure, a.json, a.iters, a.parent_lib)
        return 0
    if a.tradeoff:
        return tradeoff(os.path.join(a.log_dir, "tradeoff.md") if a.out == ap.get_default("out") else a.out, a.log_dir)
    return report(a.out, a.log_dir, a.iters, a.parent_lib)


if __name__ == "__main__":
    sys.exit(main())

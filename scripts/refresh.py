#!/usr/bin/env python3
"""Regenerate what profiles/ holds for a round on the GPU machine, as one list of steps for scripts/steps.py: each program
has its own time limit, and the first that fails ends the run.

    python scripts/refresh.py rNN [--out measure_out] [--only group[,group]] [--list]

Groups, in the order they run: tests (the GPU suite, the smoke run), bench (the bench line, the evaluation side), trace (the
bench and the two streamed shapes under a kernel trace), pmc (counter passes, each a --pmc run of its own and never beside a
trace; their summaries; traffic.json, which also reads the traces), stamps (in-kernel cycle stamps; needs ab_run/stamps.so:
scripts/mkvariants.sh stamps:"-DTLSAN_STAMPS=1"), shapes (the other shapes of BASELINE.json's configs), sharded (the
static-shape sharded step at one rank), sweep (batches of 4096 / 8192 / 16384 sequences: the data the weak-scaling
operating point of the 8-GPU step is chosen from).  --list prints name, limit and command of every
selected step and runs nothing.  Logs are <out>/rNN_<name>.log (give --out the directory that is brought back from the GPU machine); the files profiles/ takes (scripts/copy_profiles.sh)
are written beside them from the logs."""
import argparse
import json
import os
import re
import shlex
import sys

from steps import run_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("tests", "bench", "trace", "pmc", "stamps", "shapes", "sharded", "sweep")
PY = "python3"

BF16T, BF16MM = ("4096", "td=bf16"), ("4096", "td=bf16", "mm=bf16")
D256 = ("d=256", "Ls=10")
C5 = ("d=256", "Ls=90", "U=10000000", "I=5000000", "C=10000")           # tables beyond every cache
MTV = ("d=128", "Ls=90", "U=35896", "I=28589", "C=15")                   # Movies-TV with 90-entry windows

SHAPES = """
d=64 Ls=10 B=32 U=2010 I=1723 C=226
d=128 Ls=10 B=1024 U=1659 I=1583 C=53
d=128 Ls=10 B=4096
d=128 Ls=10 B=4096 sess=amazon
d=64 Ls=10 B=4096
d=64 Ls=10 B=8192
d=128 Ls=10 B=4096 U=35896 I=28589 C=15
d=128 Ls=90 B=4096 U=35896 I=28589 C=15
d=128 Ls=90 B=4096 U=35896 I=28589 C=15 sess=amazon
d=256 Ls=10 B=4096
d=256 Ls=10 B=4096 sess=amazon
d=256 Ls=90 B=4096
d=128 Ls=10 B=4096 U=10000000 I=5000000 C=10000
d=256 Ls=90 B=4096 U=10000000 I=5000000 C=10000
d=128 Ls=10 B=4096 td=bf16 mm=bf16
d=128 Ls=90 B=4096 U=35896 I=28589 C=15 td=bf16 mm=bf16
d=256 Ls=10 B=4096 td=bf16 mm=bf16
d=256 Ls=90 B=4096 td=bf16 mm=bf16
d=256 Ls=90 B=4096 U=10000000 I=5000000 C=10000 td=bf16 mm=bf16
""".strip().splitlines()

# counter sets of one --pmc pass each (the hardware takes about eight at once)
PMC_STEP = {"sq1": "SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY",
            "sq2": "SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT"}
PMC_SHAPE = {"a": "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_IFETCH",
             "b": "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_FLAT SQ_INST_CYCLES_VMEM SQ_INST_CYCLES_SALU",
             "e": "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_THREAD_CYCLES_VALU SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM SQ_INSTS_LDS",
             "c": "SQ_INSTS_SALU SQ_INSTS_VMEM SQ_INSTS_SMEM SQ_INSTS_BRANCH SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQC_ICACHE_REQ SQC_ICACHE_MISSES"}
PMC_DEEP = {"a": PMC_SHAPE["a"], "b": PMC_SHAPE["b"],
            "c": "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQC_DCACHE_REQ SQC_DCACHE_MISSES SQ_INSTS_SMEM SQ_INSTS_BRANCH",
            "d": "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_LDS_UNALIGNED_STALL SQ_LDS_MEM_VIOLATIONS SQ_INSTS_LDS SQ_LDS_ATOMIC_RETURN SQ_INSTS_VALU_MFMA_MOPS_F32",
            "e": "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_THREAD_CYCLES_VALU SQ_INST_LEVEL_LDS SQ_INST_LEVEL_VMEM SQ_WAVES_EQ_64",
            "f": "TA_BUSY_avr TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCC_HIT_sum TCC_MISS_sum",
            "g": "GRBM_GUI_ACTIVE GRBM_COUNT"}


def last_line(pattern=""):
    """the last line of a log that holds the pattern (the last line of all if none does)"""
    def pick(text):
        lines = text.splitlines() or [""]
        return ([l for l in lines if pattern in l] or lines)[-1] + "\n"
    return pick


def sharded_rate(text):
    d = json.loads(last_line('"metric"')(text))
    return "%.1f us/step, %.2f M seq/s\n" % (d["ms_per_step"] * 1e3, d["value"] / 1e6)


def step_list(tag, out="measure_out"):
    """[{group, name, argv, env, limit, cwd, save}]; save = (file suffix, text put in front or None, what of the log: a function or
    None for all of it), appended to <out>/<tag>_<suffix> when the step has succeeded"""
    G = os.path.join(out, tag)                            # (relative to the root: the post-processing steps run there)
    A = os.path.join(ROOT, out, tag)                      # (absolute: the traced and counter runs start in /tmp)
    script = lambda n: os.path.join(ROOT, "scripts", n)
    L = []

    def add(group, name, argv, limit, env=None, cwd=ROOT, save=None):
        L.append(dict(group=group, name=name, argv=[str(a) for a in argv], env=env or {}, limit=limit, cwd=cwd, save=save))

    def host(group, name, argv, save=None):               # cheap post-processing of what the group before it wrote
        add(group, name, [PY] + list(argv), 120, save=save)

    def trace(group, name, out, cmd):                     # kernel trace: a run of its own, from /tmp
        add(group, name, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", A + "_" + out, "--", PY] + list(cmd),
            600, env={"TMPDIR": "/tmp"}, cwd="/tmp")

    def pmc(name, counters, args=()):                     # counters only: never beside a trace
        add("pmc", name, ["rocprofv3", "--pmc"] + counters.split() + ["--output-format", "csv", "-d", A + "_" + name, "--", PY, script("pmc_run.py")] + list(args),
            600, env={"TMPDIR": "/tmp"}, cwd="/tmp")

    add("tests", "pytest_gpu", [PY, "-m", "pytest", "tests", "-m", "gpu", "-x", "-q"], 3000)
    add("tests", "smoke", [PY, "-c", "import __graft_entry__ as g; g.smoke(); print('smoke ok')"], 300)

    add("bench", "bench", [PY, "bench.py"], 600, save=("bench_line.json", None, last_line('"metric"')))
    add("bench", "eval_bench", [PY, "scripts/eval_bench.py"], 300, save=("eval_bench.txt", None, None))

    trace("trace", "bench_under_rocprof", "stats", [os.path.join(ROOT, "bench.py"), "--no-cpu-baseline"])
    trace("trace", "streamed_stats", "streamed_stats", [script("shape_bench.py")] + list(MTV[:2]) + ["B=4096"] + list(MTV[2:]))
    trace("trace", "c5_stats", "c5_stats", [script("shape_bench.py")] + list(C5[:2]) + ["B=4096"] + list(C5[2:]))
    host("trace", "kstats", ["scripts/kstats.py", G + "_stats", 8])
    host("trace", "kstats_streamed", ["scripts/kstats.py", G + "_streamed_stats", 8], save=("streamed_kernel_stats.txt", "# Movies-TV shape, Ls = 90\n", None))
    host("trace", "kstats_c5", ["scripts/kstats.py", G + "_c5_stats", 10], save=("streamed_kernel_stats.txt", "# C5 shape\n", None))

    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        pmc(c, c)
        # the same in the precisions BASELINE.json configs[2] names: bf16 tables, bf16 tables + bf16 matrix operands
        pmc(c + "_bf16t", c, BF16T)
        pmc(c + "_bf16mm", c, BF16MM)
        # ... and at the two shapes whose step is not the bench's
        pmc(c + "_c5", c, ("4096",) + C5)
        pmc(c + "_mtv", c, ("4096",) + MTV)
    for n, counters in PMC_STEP.items():
        pmc(n, counters)
    host("pmc", "pmc_summary_step", ["scripts/pmc_summary.py"] + [G + "_" + n for n in ("FETCH_SIZE", "WRITE_SIZE", "sq1", "sq2")],
         save=("pmc_summary.txt", None, None))
    for t, shape in (("pmc_d256", D256), ("pmc_c5", C5), ("pmc_streamed", MTV)):
        for n, counters in PMC_SHAPE.items():
            pmc("%s_%s" % (t, n), counters, shape)
        host("pmc", t + "_sum", ["scripts/pmc_summary.py"] + ["%s_%s_%s" % (G, t, n) for n in PMC_SHAPE], save=(t + "_summary.txt", None, None))
    add("pmc", "pmc_deep_counters", ["rocprofv3", "-L"], 600, env={"TMPDIR": "/tmp"}, cwd="/tmp", save=("pmc_deep_counters.txt", None, None))
    for n, counters in PMC_DEEP.items():
        pmc("pmc_deep_" + n, counters)
    host("pmc", "pmc_deep_sum", ["scripts/pmc_summary.py"] + ["%s_pmc_deep_%s" % (G, n) for n in PMC_DEEP], save=("pmc_deep_summary.txt", None, None))
    # (the traffic nodes of the C5 / Movies-TV shapes take their kernel durations from the traces of the group before)
    host("pmc", "traffic_json", ["scripts/traffic_json.py", tag[1:], G], save=("traffic.json", None, None))

    stamps_lib = {"TLSAN_LIB_PATH": os.path.join(ROOT, "ab_run", "stamps.so")}
    add("stamps", "stamps", [PY, "scripts/stamps.py"], 300, env=stamps_lib, save=("stamps.txt", None, None))
    add("stamps", "stamps_bf16", [PY, "scripts/stamps.py"], 300, env={**stamps_lib, "MM": "bf16", "TD": "bf16"}, save=("stamps_bf16.txt", None, None))
    add("stamps", "stamps_streamed", [PY, "scripts/stamps.py"] + list(MTV), 300, env=stamps_lib, save=("stamps_streamed.txt", None, None))

    for i, shape in enumerate(SHAPES, 1):
        add("shapes", "shape%02d" % i, [PY, "scripts/shape_bench.py"] + shape.split(), 600,
            save=("shapes.txt", "# scripts/shape_bench.py %s\n" % shape, last_line()))

    trace("sharded", "shard_static", "shard_static", [script("shard_static_prof.py")])
    host("sharded", "kstats_shard_static", ["scripts/kstats.py", G + "_shard_static", 14], save=("sharded_static_kernel_stats.txt", None, None))
    sharded = [PY, "bench.py", "--force-sharded", "--no-cpu-baseline", "--accuracy-steps", "0"]
    add("sharded", "sharded_bench", sharded, 300, env={"AHEAD": "2"}, save=("sharded_bench_line.json", None, last_line('"metric"')))

    for B in (4096, 8192, 16384):
        for p, prec in (("f32", []), ("bf16", ["td=bf16", "mm=bf16"])):
            add("sweep", "sweep_B%d_%s" % (B, p), [PY, "scripts/shape_bench.py", "d=128", "Ls=10", "B=%d" % B] + prec, 300,
                save=("batch_sweep.txt", None, last_line()))
        add("sweep", "sweep_B%d_sharded" % B, sharded + ["--batch", B], 300, env={"AHEAD": "2"},
            save=("batch_sweep.txt", "one-rank sharded step (static rows, plans two ahead), B=%d: " % B, sharded_rate))
    return L


def main(argv=None, out=None):
    out = out or sys.stdout
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tag", help="the round, rNN: every output is <out>/rNN_*")
    ap.add_argument("--out", default="measure_out", help="directory of the logs and results, from the repository's root")
    ap.add_argument("--only", default=",".join(GROUPS), help="groups to run, of: " + " ".join(GROUPS))
    ap.add_argument("--list", action="store_true", help="print name, limit and command of every selected step; run nothing")
    args = ap.parse_args(argv)
    only = args.only.split(",")
    if not re.fullmatch(r"r\d+", args.tag) or set(only) - set(GROUPS):
        ap.error("the tag is rNN; groups are: " + " ".join(GROUPS))
    L = [s for g in GROUPS if g in only for s in step_list(args.tag, args.out) if s["group"] == g]
    if args.list:
        for s in L:
            env = "".join("%s=%s " % kv for kv in s["env"].items())
            print("%-8s %-28s %5d  %s%s" % (s["group"], s["name"], s["limit"], env, shlex.join(s["argv"])), file=out)
        return 0
    log_dir = os.path.join(ROOT, args.out)
    saved = {s["name"]: s["save"] for s in L if s["save"]}
    dest = lambda suffix: os.path.join(log_dir, "%s_%s" % (args.tag, suffix))
    for suffix in set(sv[0] for sv in saved.values()):
        if os.path.exists(dest(suffix)):
            os.remove(dest(suffix))      # (they are appended to below)

    def done(step, text):
        name = step[0][len(args.tag) + 1:]
        print("done: %s" % name, file=out, flush=True)
        if name in saved:
            suffix, header, pick = saved[name]
            with open(dest(suffix), "a") as f:
                f.write((header or "") + (pick(text) if pick else text))

    return run_steps([("%s_%s" % (args.tag, s["name"]), s["argv"], s["env"], s["limit"], s["cwd"]) for s in L], log_dir, on_done=done, out=out)


if __name__ == "__main__":
    sys.exit(main())

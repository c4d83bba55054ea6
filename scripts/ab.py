#!/usr/bin/env python3
"""Interleaved rounds of one command over variants on ONE GPU machine (step times differ between machines by more than
most changes are worth), then, if asked, one kernel-trace pass per variant.  Every program is a step of scripts/steps.py:
each has its own time limit, and the first that fails ends the measurement.

    python scripts/ab.py [--rounds 3] [--limit 300] [--trace] [--top 8] [--out measure_out/ab]
                         [--libs [DIR]] [--env VAR=v1,v2,...] [--variant NAME,KEY=VAL,...]...
                         [-- command...]

Variants: --libs, one per DIR/*.so (default ab_run/, built by scripts/mkvariants.sh), loaded through TLSAN_LIB_PATH so that
the in-tree library is never overwritten; --env, one per value of one variable; --variant, named explicitly; none of these,
the tree as built.  The command defaults to the fp32 leg of the bench; a path in it is taken from the repository's root.
A round runs every variant once (A B A B A B).  Of a run, the bench's JSON line is read if there is one, else the last line
holding `us/step` (of a command that prints neither, the last line is shown and nothing is summed); the summary gives
min / median / max of the step time per variant and the final losses.  --trace runs every variant once more under
`rocprofv3 --kernel-trace --stats` from /tmp, only after all timed runs succeeded, and prints the top kernels
(scripts/kstats.py): tracing never rides on a timed run.

What the runner scripts this replaces did, as one invocation each:
    ab.sh <commit> [args]           scripts/mkvariants.sh rev:<commit>   (where the tree is built), then
                                    ab.py --libs -- python bench.py --no-cpu-baseline --accuracy-steps 0 --also-bf16 0 [args]
    abrun.sh N                      ab.py --rounds N --libs
    abrun2.sh N, abrun3.sh N        ab.py --rounds N --libs -- python bench.py --no-cpu-baseline --accuracy-steps 0 --also-bf16 1
    abshape.sh N shape...           ab.py --rounds N --libs -- python scripts/shape_bench.py shape...
    shape_ab.sh N shape...          the same
    envab.sh VAR "v1 v2" N          ab.py --rounds N --env VAR=v1,v2
    envab_shape.sh VAR "v1 v2" N shape...
                                    ab.py --rounds N --env VAR=v1,v2 -- python scripts/shape_bench.py shape...
    bench_repeat.sh N               ab.py --rounds N
    kstats_shape.sh tag shape...    ab.py --rounds 1 --trace -- python scripts/shape_bench.py shape...
    shape_kstats.sh shape...        ab.py --rounds 1 --trace --top 6 --libs -- python scripts/shape_bench.py shape...
    env_kstats.sh VAR "v1 v2" shape...
                                    ab.py --rounds 1 --trace --top 7 --env VAR=v1,v2 -- python scripts/shape_bench.py shape...
    kprof.sh name [args]            ab.py --rounds 1 --trace --top 9 --out measure_out/name
                                          -- python bench.py --no-cpu-baseline --accuracy-steps 0 [args]
"""
import argparse
import glob
import json
import os
import re
import shlex
import shutil
import statistics
import sys

from steps import run_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["python", "bench.py", "--no-cpu-baseline", "--accuracy-steps", "0", "--also-bf16", "0"]
TRACE_LIMIT = 600


def variants(args):
    """[(name, env_overrides)]"""
    vs = []
    if args.libs:
        d = os.path.join(ROOT, args.libs)
        vs += [(os.path.basename(so)[:-3], {"TLSAN_LIB_PATH": os.path.abspath(so)}) for so in sorted(glob.glob(os.path.join(d, "*.so")))]
        if not vs:
            sys.exit("ab.py: no library in %s" % d)
    if args.env:
        var, vals = args.env.split("=", 1)
        vs += [("%s=%s" % (var, v), {var: v}) for v in vals.split(",")]
    for spec in args.variant:
        name, *kvs = spec.split(",")
        vs.append((name, dict(kv.split("=", 1) for kv in kvs)))
    return vs or [("tree", {})]


def read_run(text):
    """What one run's log says: {"us": step time, "loss": ..., "line": the line to print}"""
    lines = text.splitlines()
    for l in reversed(lines):
        if '"metric"' in l:
            d = json.loads(l[l.index("{"):])
            r = {"us": d["ms_per_step"] * 1e3, "loss": d["final_loss"]}
            r["line"] = "step %.2f us  k_fwd_bwd %.2f us  loss %s" % (r["us"], d["roofline"]["kernel_ms"] * 1e3, r["loss"])
            if "bf16_mfma" in d:
                b = d["bf16_mfma"]
                r["loss"] = (r["loss"], b["final_loss"])
                r["line"] += " | bf16 step %.2f us  k_fwd_bwd %.2f us  loss %s" % (b["ms_per_step"] * 1e3, b["roofline"]["kernel_ms"] * 1e3, b["final_loss"])
            return r
    for l in reversed(lines):
        if "us/step" in l:
            us, loss = re.search(r"([0-9.]+) us/step", l), re.search(r"loss (\S+)", l)
            return {"us": float(us.group(1)) if us else None, "loss": loss.group(1) if loss else None, "line": l}
    return {"us": None, "loss": None, "line": next((l for l in reversed(lines) if l.strip()), "(nothing in the log)")}   # (a command that is no bench)


def summary(names, runs, out):
    """runs: {variant: [read_run result per round]}"""
    print("\n%-24s %3s %10s %10s %10s   %s" % ("variant", "n", "min us", "median us", "max us", "final loss"), file=out)
    losses = {}
    for n in names:
        us = [r["us"] for r in runs[n] if r["us"] is not None]
        losses[n] = sorted(set(r["loss"] for r in runs[n]), key=str)
        stat = "%10.2f %10.2f %10.2f" % (min(us), statistics.median(us), max(us)) if us else "%10s %10s %10s" % ("-", "-", "-")
        print("%-24s %3d %s   %s" % (n, len(runs[n]), stat, " ".join(str(l) for l in losses[n])), file=out)
    if len(names) > 1:
        same = all(losses[n] == losses[names[0]] for n in names)
        print("final losses: %s" % ("the same for every variant" if same else "DIFFER between variants"), file=out)


def main(argv=None, out=None):
    out = out or sys.stdout
    argv = list(sys.argv[1:] if argv is None else argv)
    command = BENCH
    if "--" in argv:
        command = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds for one timed run")
    ap.add_argument("--trace", action="store_true", help="after the timed rounds, one kernel-trace run per variant")
    ap.add_argument("--top", type=int, default=8, help="kernels printed per traced variant")
    ap.add_argument("--out", default=os.path.join("measure_out", "ab"), help="directory of the logs and traces")
    ap.add_argument("--libs", nargs="?", const="ab_run", metavar="DIR")
    ap.add_argument("--env", metavar="VAR=v1,v2,...")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME,KEY=VAL,...")
    ap.add_argument("--tracer", default="rocprofv3", help="the tracing program (tests put a stand-in here)")
    args = ap.parse_args(argv)
    if not command:
        ap.error("no command after --")
    # the traced runs start in /tmp, so a path in the command is made absolute (for the timed runs too: one command)
    command = [os.path.join(ROOT, a) if os.path.isfile(os.path.join(ROOT, a)) else a for a in command]
    vs = variants(args)
    names = [n for n, _ in vs]
    if len(set(names)) != len(names):
        sys.exit("ab.py: two variants with one name: %s" % " ".join(names))
    log_dir = os.path.join(ROOT, args.out)
    safe = {n: re.sub(r"[^A-Za-z0-9_.+-]", "_", n) for n in names}

    runs = {n: [] for n in names}
    timed, whose = [], {}
    for r in range(1, args.rounds + 1):
        for n, env in vs:
            timed.append(("round%d_%s" % (r, safe[n]), command, env, args.limit, ROOT))
            whose[timed[-1][0]] = n

    def timed_done(step, text):
        res = read_run(text)
        runs[whose[step[0]]].append(res)
        print("%-24s %s" % (whose[step[0]], res["line"]), file=out, flush=True)

    rc = run_steps(timed, log_dir, on_done=timed_done, out=out)
    if rc != 0:
        print("the measurement ended at its first failed run: no summary, no trace", file=out)
        return rc
    summary(names, runs, out)
    if not args.trace:
        return 0

    traced, env_tmp = [], {"TMPDIR": "/tmp"}
    for n, env in vs:
        d = os.path.join(log_dir, safe[n])
        shutil.rmtree(d, ignore_errors=True)   # (kstats.py reads the first stats file it finds: none of an earlier pass)
        traced.append(("trace_" + safe[n], shlex.split(args.tracer) + ["--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + command,
                       {**env, **env_tmp}, TRACE_LIMIT, "/tmp"))
        traced.append(("kstats_" + safe[n], ["python", os.path.join(ROOT, "scripts", "kstats.py"), d, str(args.top)], {}, 60, ROOT))
        whose[traced[-2][0]] = whose[traced[-1][0]] = n

    def traced_done(step, text):
        if step[0].startswith("trace_"):
            print("\n== %s, traced: %s" % (whose[step[0]], read_run(text)["line"]), file=out)
        else:
            print(text, end="", file=out, flush=True)

    return run_steps(traced, log_dir, on_done=traced_done, out=out)


if __name__ == "__main__":
    sys.exit(main())

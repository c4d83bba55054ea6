#!/usr/bin/env python3
"""The one place that starts the programs of a GPU measurement: one after another, each under its own time limit, and
nothing more after the first that fails.

    from steps import run_steps
    rc = run_steps([(name, argv, env_overrides, limit_seconds, cwd), ...], log_dir)

A step is started as `timeout -k 10 <limit> argv...` (the limit holds even if this process is killed) with the caller's
environment plus its own env_overrides; stdout and stderr go to log_dir/<name>.log.  It failed when its status is not 0, or
when its log holds HIP's report of a GPU fault, which some programs survive.  After a failure nothing more is started: there
is no retry and no way to go on.  scripts/ab.py and scripts/refresh.py are lists of steps on top of this."""
import os
import subprocess
import sys

FAULT_TEXT = "an illegal memory access was encountered"
MEANING = {124: "time limit", 137: "time limit (killed)", 134: "abort", -6: "abort", 139: "segmentation fault", -11: "segmentation fault"}


def log_path(log_dir, name):
    return os.path.join(log_dir, name + ".log")


def run_steps(steps, log_dir, on_done=None, out=None):
    """Run the steps in order; 0 when all succeeded, else the status of the one that failed (1 for a fault found in the log
    of a step that exited 0).  on_done(step, log_text), if given, is called after each step that succeeded."""
    out = out or sys.stdout
    os.makedirs(log_dir, exist_ok=True)
    for step in steps:
        name, argv, env, limit, cwd = step
        path = log_path(log_dir, name)
        with open(path, "wb") as log:
            rc = subprocess.run(["timeout", "-k", "10", str(limit)] + [str(a) for a in argv], env={**os.environ, **(env or {})},
                                cwd=cwd, stdin=subprocess.DEVNULL, stdout=log, stderr=subprocess.STDOUT).returncode
        with open(path, errors="replace") as log:
            text = log.read()
        fault = FAULT_TEXT in text
        if rc != 0 or fault:
            what = MEANING.get(rc, "GPU fault reported in its log" if rc == 0 else "failed")
            print("step %s FAILED: status %d (%s%s); nothing more is started" % (
                name, rc, what, ", and a GPU fault reported in its log" if fault and rc != 0 else ""), file=out)
            print("--- last lines of %s" % path, file=out)
            print("\n".join(text.splitlines()[-30:]), file=out, flush=True)
            return rc if rc != 0 else 1
        if on_done:
            on_done(step, text)
    return 0

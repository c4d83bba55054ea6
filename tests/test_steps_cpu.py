"""The measurement tooling on the CPU: scripts/steps.py runs steps in order and starts nothing after the first that fails;
scripts/ab.py interleaves variants and summarises them; scripts/refresh.py lists the profile set.  Every child is a small
python program; nothing here touches a GPU."""
import io
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)
import steps  # noqa: E402

PY = sys.executable


def touch(path, then=""):
    """argv of a child that creates `path`, then runs `then`"""
    return [PY, "-c", "import os, sys, time; open(%r, 'w').close(); %s" % (str(path), then or "pass")]


def run(step_list, tmp_path):
    out = io.StringIO()
    return steps.run_steps(step_list, str(tmp_path / "logs"), out=out), out.getvalue()


def test_three_steps_run_in_order(tmp_path):
    order = tmp_path / "order"
    mark = lambda n: [PY, "-c", "open(%r, 'a').write('%s\\n'); print('step %s')" % (str(order), n, n)]
    rc, msg = run([(n, mark(n), {}, 30, None) for n in ("a", "b", "c")], tmp_path)
    assert rc == 0 and msg == ""
    assert order.read_text().split() == ["a", "b", "c"]
    for n in ("a", "b", "c"):
        assert (tmp_path / "logs" / (n + ".log")).read_text() == "step %s\n" % n


@pytest.mark.parametrize("status, meaning", [(139, "segmentation fault"), (134, "abort")])
def test_nothing_starts_after_a_failed_step(tmp_path, status, meaning):
    m = [tmp_path / n for n in "abc"]
    rc, msg = run([("first", touch(m[0]), {}, 30, None),
                   ("second", touch(m[1], "print('the end of it'); sys.exit(%d)" % status), {}, 30, None),
                   ("third", touch(m[2]), {}, 30, None)], tmp_path)
    assert rc == status
    assert m[0].exists() and m[1].exists() and not m[2].exists()
    assert "second" in msg and str(status) in msg and meaning in msg and "the end of it" in msg
    assert not (tmp_path / "logs" / "third.log").exists()


def test_signals_have_the_same_meaning(tmp_path):
    # (a child that dies of the signal itself: `timeout` then ends itself with that signal, and the status is its negative)
    rc, msg = run([("dies", [PY, "-c", "import os, signal; os.kill(os.getpid(), signal.SIGABRT)"], {}, 30, None)], tmp_path)
    assert rc == -6 and "-6 (abort)" in msg
    assert steps.MEANING[-6] == steps.MEANING[134] and steps.MEANING[-11] == steps.MEANING[139] == "segmentation fault"


def test_time_limit_ends_the_run(tmp_path):
    m = [tmp_path / n for n in "ab"]
    rc, msg = run([("sleeper", touch(m[0], "time.sleep(30)"), {}, 1, None), ("after", touch(m[1]), {}, 30, None)], tmp_path)
    assert rc == 124
    assert m[0].exists() and not m[1].exists()
    assert "sleeper" in msg and "124" in msg and "time limit" in msg


def test_fault_text_fails_a_step_that_exits_zero(tmp_path):
    m = [tmp_path / n for n in "ab"]
    rc, msg = run([("faulty", touch(m[0], "print('HIP error: an illegal memory access was encountered'); print('went on')"), {}, 30, None),
                   ("after", touch(m[1]), {}, 30, None)], tmp_path)
    assert rc == 1
    assert m[0].exists() and not m[1].exists()
    assert "faulty" in msg and "an illegal memory access was encountered" in msg


def test_env_overrides_hold_for_their_step_only(tmp_path):
    show = [PY, "-c", "import os; print(os.environ.get('STEPS_TEST_VAR', 'unset'), os.environ.get('HOME', 'nohome'))"]
    assert "STEPS_TEST_VAR" not in os.environ
    rc, _ = run([("with", show, {"STEPS_TEST_VAR": "7"}, 30, None), ("without", show, {}, 30, None)], tmp_path)
    assert rc == 0
    home = os.environ.get("HOME", "nohome")     # (the caller's environment is passed on)
    assert (tmp_path / "logs" / "with.log").read_text().split() == ["7", home]
    assert (tmp_path / "logs" / "without.log").read_text().split() == ["unset", home]
    assert "STEPS_TEST_VAR" not in os.environ


# --- scripts/ab.py over a stand-in for the bench: the step time is FAKE_US plus an offset per round, all from the environment

FAKE = textwrap.dedent("""
    import json, os, sys
    order = os.environ["FAKE_ORDER"]
    calls = len(open(order).read().split()) if os.path.exists(order) else 0
    open(order, "a").write(os.environ.get("FAKE_NAME", "tree") + "\\n")
    if str(calls) == os.environ.get("FAKE_FAIL_AT"):
        sys.exit(3)
    us = float(os.environ.get("FAKE_US", "50")) + (0.5, 0.1, 0.3)[calls // 2 % 3]
    print("some warning on the way", file=sys.stderr)
    if "text" in sys.argv[1:]:
        print("warm-up took 3.0 us/step")
        print("d=128 Ls=10 B=4096: %.1f us/step, 1.00 M seq/s, loss 0.6931" % us)
    else:
        print(json.dumps({"metric": "fake", "ms_per_step": us / 1e3, "final_loss": float(os.environ.get("FAKE_LOSS", "0.5")),
                          "roofline": {"kernel_ms": 0.03}}))
""")

TRACER = textwrap.dedent("""
    import os, subprocess, sys
    a = sys.argv[1:]
    assert a[:4] == ["--kernel-trace", "--stats", "--output-format", "csv"] and a[4] == "-d" and a[6] == "--", a
    assert os.getcwd() == "/tmp" and os.environ["TMPDIR"] == "/tmp"
    open(os.environ["FAKE_ORDER"], "a").write("trace\\n")
    os.makedirs(os.path.join(a[5], "host"))
    with open(os.path.join(a[5], "host", "1_kernel_stats.csv"), "w") as f:
        f.write("Name,Calls,AverageNs,Percentage\\nk_of_%s,12,34000,99.0\\n" % os.environ.get("FAKE_NAME", "tree"))
    sys.exit(subprocess.run(a[7:]).returncode)
""")

AB_VARIANTS = ["--variant", "A,FAKE_NAME=A,FAKE_US=50", "--variant", "B,FAKE_NAME=B,FAKE_US=60,FAKE_LOSS=0.5"]


def ab(tmp_path, *args, command=(), env=None):
    fake, tracer = tmp_path / "fake.py", tmp_path / "tracer.py"
    fake.write_text(FAKE)
    tracer.write_text(TRACER)
    r = subprocess.run([PY, os.path.join(SCRIPTS, "ab.py"), "--out", str(tmp_path / "out"), "--tracer", "%s %s" % (PY, tracer), *args,
                        "--", PY, str(fake), *command],
                       env={**os.environ, "FAKE_ORDER": str(tmp_path / "order"), **(env or {})}, capture_output=True, text=True, timeout=120)
    order = (tmp_path / "order").read_text().split() if (tmp_path / "order").exists() else []
    return r, order


def table(stdout):
    """{variant: [n, min, median, max, losses...]} of the summary"""
    lines = stdout.splitlines()
    at = next(i for i, l in enumerate(lines) if l.startswith("variant"))
    return {l.split()[0]: l.split()[1:] for l in lines[at + 1:] if l and not l.startswith("final losses")}


def test_ab_interleaves_and_summarises(tmp_path):
    r, order = ab(tmp_path, "--rounds", "3", *AB_VARIANTS)
    assert r.returncode == 0, r.stdout + r.stderr
    assert order == ["A", "B", "A", "B", "A", "B"]
    runs = [l for l in r.stdout.splitlines() if " step " in l and "k_fwd_bwd" in l]
    assert [l.split()[0] for l in runs] == order                       # one line per run, as they finished
    assert "step 50.50 us  k_fwd_bwd 30.00 us  loss 0.5" in runs[0]
    t = table(r.stdout)
    assert t["A"] == ["3", "50.10", "50.30", "50.50", "0.5"]
    assert t["B"] == ["3", "60.10", "60.30", "60.50", "0.5"]
    assert "final losses: the same for every variant" in r.stdout


def test_ab_says_when_losses_differ(tmp_path):
    r, _ = ab(tmp_path, "--rounds", "1", "--variant", "A,FAKE_NAME=A", "--variant", "B,FAKE_NAME=B,FAKE_LOSS=0.25")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFER" in r.stdout and "the same for every variant" not in r.stdout


def test_ab_without_variants_repeats_the_tree(tmp_path):
    r, order = ab(tmp_path, "--rounds", "2")
    assert r.returncode == 0, r.stdout + r.stderr
    assert order == ["tree", "tree"]
    assert table(r.stdout)["tree"][0] == "2"


def test_ab_env_variants(tmp_path):
    r, order = ab(tmp_path, "--rounds", "2", "--env", "FAKE_NAME=x,y")
    assert r.returncode == 0, r.stdout + r.stderr
    assert order == ["x", "y", "x", "y"]
    assert set(table(r.stdout)) == {"FAKE_NAME=x", "FAKE_NAME=y"}


def test_ab_libs_variants(tmp_path):
    libs = tmp_path / "libs"
    libs.mkdir()
    for n in ("new.so", "base.so", "notes.txt"):
        (libs / n).write_text("")
    show = tmp_path / "show.py"
    show.write_text("import os; print(os.environ['TLSAN_LIB_PATH'], '1.0 us/step')")
    r = subprocess.run([PY, os.path.join(SCRIPTS, "ab.py"), "--out", str(tmp_path / "out"), "--rounds", "1", "--libs", str(libs), "--", PY, str(show)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    runs = [l.split() for l in r.stdout.splitlines() if "us/step" in l]
    assert [(l[0], l[1]) for l in runs] == [("base", str(libs / "base.so")), ("new", str(libs / "new.so"))]   # sorted, absolute


def test_ab_keeps_a_us_per_step_line_verbatim(tmp_path):
    r, order = ab(tmp_path, "--rounds", "3", *AB_VARIANTS, command=["text"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert order == ["A", "B"] * 3
    kept = "d=128 Ls=10 B=4096: 50.5 us/step, 1.00 M seq/s, loss 0.6931"
    assert [l for l in r.stdout.splitlines() if l.endswith(kept)] == ["%-24s %s" % ("A", kept)]
    assert "warm-up" not in r.stdout
    assert table(r.stdout)["B"] == ["3", "60.10", "60.30", "60.50", "0.6931"]


def test_ab_ends_at_a_failed_run(tmp_path):
    r, order = ab(tmp_path, "--rounds", "3", "--trace", *AB_VARIANTS, env={"FAKE_FAIL_AT": "3"})   # B in round 2
    assert r.returncode == 3
    assert order == ["A", "B", "A", "B"]                                # no round 3, no trace
    assert "round2_B" in r.stdout and "nothing more is started" in r.stdout
    assert not any(l.startswith("variant") for l in r.stdout.splitlines())


def test_ab_traces_after_all_timed_runs(tmp_path):
    r, order = ab(tmp_path, "--rounds", "2", "--trace", "--top", "3", *AB_VARIANTS)
    assert r.returncode == 0, r.stdout + r.stderr
    assert order == ["A", "B", "A", "B", "trace", "A", "trace", "B"]
    assert r.stdout.index("median us") < r.stdout.index("k_of_A") < r.stdout.index("k_of_B")
    assert table(r.stdout.split("\n==")[0])["A"][0] == "2"             # the traced run is in no statistic


# --- scripts/refresh.py --list

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


def refresh_list(*args):
    r = subprocess.run([PY, os.path.join(SCRIPTS, "refresh.py"), "r99", "--list", *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [l.split(None, 3) for l in r.stdout.splitlines()]     # group, name, limit, command


def test_refresh_list_limits_and_counter_passes():
    rows = refresh_list()
    assert {g for g, *_ in rows} == {"tests", "bench", "trace", "pmc", "stamps", "shapes", "sharded", "sweep"}
    assert len({n for _, n, *_ in rows}) == len(rows)              # one log per step
    for group, name, limit, command in rows:
        assert int(limit) > 0, name
        if "--pmc" in command.split():
            assert not any(w.startswith("--") and w.endswith("-trace") for w in command.split()), name
            assert group == "pmc"
    assert sum("--pmc" in c.split() for *_, c in rows) == 31       # 10 traffic + 2 step + 3 x 4 shape + 7 deep
    assert sum("--kernel-trace" in c.split() for *_, c in rows) == 4


def test_refresh_only_shapes_is_the_nineteen_shapes():
    rows = refresh_list("--only", "shapes")
    assert [c.split("shape_bench.py ", 1)[1] for *_, c in rows] == SHAPES
    assert all(g == "shapes" and int(limit) == 600 for g, _, limit, _ in rows)


def test_refresh_without_a_tag_is_an_error():
    r = subprocess.run([PY, os.path.join(SCRIPTS, "refresh.py"), "--list"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0

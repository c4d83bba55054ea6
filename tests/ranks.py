"""The one place that starts the ranks of a multi-process test.

    values = run_ranks(fn, world, *args, backend="gloo", timeout=600, grace=30, env=None)

runs fn(rank, world, *args) in `world` fresh processes ("spawn") that form one process group, and returns what the ranks
returned, in rank order.  fn is a module-level function (pickled by reference).  Trouble ends the call: a rank that raises,
exits without a report or is killed by a signal gives the others `grace` seconds to end by themselves, after which they
are terminated; at `timeout` seconds every rank is.  No process outlives the call, whatever its outcome, and any of these
raises one AssertionError with a line per rank.  Nothing is started again after a failure."""
import multiprocessing
import os
import pickle
import socket
import time
import traceback
from multiprocessing.connection import wait


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _child(fn, rank, world, args, backend, port, env, conn):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **(env or {}))
        kw = {}
        if backend == "nccl":       # one GPU per rank
            import torch
            torch.cuda.set_device(rank)
            kw["device_id"] = torch.device("cuda:%d" % rank)
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
        report = ("ok", fn(rank, world, *args))
        pickle.dumps(report)
    except BaseException:           # (pytest's own outcomes, which a worker may raise, are no Exception)
        report = ("fail", traceback.format_exc())
    conn.send(report)               # before the teardown: one that gets stuck cannot lose it
    conn.close()
    if dist.is_initialized():
        dist.destroy_process_group()


def _stop(procs):
    """terminate what is still alive, kill 10 s later what did not go, join everything"""
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.terminate()
    end = time.monotonic() + 10
    for p in alive:
        p.join(max(0.0, end - time.monotonic()))
    for p in alive:
        if p.is_alive():
            p.kill()
    for p in procs:
        p.join()


def run_ranks(fn, world, *args, backend="gloo", timeout=600, grace=30, env=None):
    pickle.dumps(fn)                # a lambda or a nested function fails here, before anything is started
    ctx = multiprocessing.get_context("spawn")
    port = free_port()
    reports, conns, procs = {}, {}, []
    try:
        for rank in range(world):
            recv, send = ctx.Pipe(duplex=False)
            p = ctx.Process(target=_child, args=(fn, rank, world, args, backend, port, env, send))
            p.start()
            send.close()            # (the child holds the writing end now: its exit closes the pipe)
            procs.append(p)
            conns[recv] = rank
        sentinels = {p.sentinel: rank for rank, p in enumerate(procs)}
        deadline, limit = time.monotonic() + timeout, "timeout"
        while sentinels:
            left = deadline - time.monotonic()
            ready = wait(list(conns) + list(sentinels), left) if left > 0 else []
            if not ready:
                break
            for r in ready:
                if r in conns:
                    try:
                        reports[conns[r]] = r.recv()
                    except EOFError:        # closed without a report
                        pass
                    del conns[r]
                    r.close()
            for r in ready:
                if r in sentinels:
                    rank = sentinels.pop(r)
                    # (the sentinel is a pipe the exiting process closes with its other files, the GPU's among them, some
                    #  time before it can be reaped: wait for the exit code itself)
                    procs[rank].join(max(0.0, deadline - time.monotonic()))
                    for c in [c for c, k in conns.items() if k == rank]:    # a report sent just before the exit
                        if c.poll():
                            reports[rank] = c.recv()
                        del conns[c]
                        c.close()
            bad = any(v[0] == "fail" for v in reports.values()) or \
                any(p.exitcode is not None and (p.exitcode != 0 or rank not in reports) for rank, p in enumerate(procs))
            if bad and limit == "timeout":  # the first bad event: the others get `grace` seconds, within the limit
                deadline, limit = min(deadline, time.monotonic() + grace), "grace"
        overran = [p.is_alive() for p in procs]
    finally:
        _stop(procs)
        for c in conns:
            c.close()
    lines, failed = [], False
    for rank, p in enumerate(procs):
        kind, value = reports.get(rank, ("none", None))
        if kind == "fail":
            what = value
        elif overran[rank]:
            what = "killed at the %g s limit" % timeout if limit == "timeout" else \
                "killed %g s after another rank had failed" % grace
            what += " (had reported ok)" if kind == "ok" else ""
        elif p.exitcode != 0:
            what = "signal %d" % -p.exitcode if p.exitcode < 0 else "exit code %d" % p.exitcode
        else:
            what = "ok" if kind == "ok" else "no report"
        failed = failed or what != "ok"
        lines.append("rank %d: %s" % (rank, what))
    assert not failed, "\n".join(lines)
    return [reports[rank][1] for rank in range(world)]

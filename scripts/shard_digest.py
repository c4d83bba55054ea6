"""One sha256 per configuration of the sharded driver over the float32 bytes of the losses, gather_params() and
gather_slots() after 8 steps: two commits that print the same digests on the same machine compute the same bits.
Public surface of ShardedModel only (the file runs unchanged on an older checkout).  One- and two-rank gloo groups on
one GPU, each in spawned children."""
import hashlib
import os
import socket
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS, LR, WEIGHTS = 8, 0.7, (1.0, 0.5, 1.0, 0.25)

# name -> (config overrides, constructor arguments, run options)
ONE_RANK = [
    ("dense sgd", {}, dict(l2_mode="dense"), {}),
    ("dense adam", dict(optimizer="adam"), dict(l2_mode="dense"), {}),
    ("lazy sgd", {}, dict(l2_mode="lazy"), {}),
    ("lazy_adam", dict(optimizer="lazy_adam"), dict(l2_mode="lazy"), {}),
    ("static, two ahead", {}, dict(l2_mode="lazy", static_rows=True), dict(ahead=2)),
    ("static, fixed capacity", {}, dict(l2_mode="lazy", static_rows=2048), dict(ahead=2)),
    ("static, bf16 wire", {}, dict(l2_mode="lazy", static_rows=True, wire_dtype="bf16"), dict(ahead=2)),
    ("static, 4 eager + 4 captured", {}, dict(l2_mode="lazy", static_rows=True), dict(ahead=1, graphs=True)),
    ("dynamic, weights", {}, dict(l2_mode="lazy"), dict(weights=True)),
    ("static, weights", {}, dict(l2_mode="lazy", static_rows=True), dict(ahead=2, weights=True)),
    ("dynamic, dropout", dict(dropout=0.1), dict(l2_mode="lazy"), dict(sample0=24)),
    ("static, dropout", dict(dropout=0.1), dict(l2_mode="lazy", static_rows=True), dict(ahead=2, sample0=24)),
]
TWO_RANKS = [
    ("2 ranks: lazy dynamic", {}, dict(l2_mode="lazy"), {}),
    ("2 ranks: static, deferred_ids", {}, dict(l2_mode="lazy", static_rows=True, deferred_ids=True), dict(ahead=2)),
    ("2 ranks: static, coalesce", {}, dict(l2_mode="lazy", static_rows=True, coalesce=True), dict(ahead=2)),
]


def digest(losses, params, slots):
    h = hashlib.sha256()
    h.update(np.asarray(losses, np.float32).tobytes())
    for d in [params] + list(slots or []):
        for k in sorted(d):
            h.update(k.encode())
            h.update(np.ascontiguousarray(np.asarray(d[k], np.float32)).tobytes())
    return h.hexdigest()


def run_one(rank, world, over, ctor, ahead=1, graphs=False, weights=False, sample0=0):
    from tlsan_amd import synth
    from tlsan_amd.dist import ShardedModel
    cfg = synth.make_config("electronics", user_count=3001, item_count=2203, cate_count=67, **over)
    icl = synth.item_cate_list(cfg)
    if world == 1:
        batches = synth.make_batches(cfg, 4, 256, seed=5, sessions="amazon")
    else:
        batches = [synth.make_batches(cfg, 1, 256, seed=700 + 10 * s + rank, sessions="amazon")[0] for s in range(4)]
    m = ShardedModel(cfg, icl, device="cuda:0", **ctor)
    static = bool(ctor.get("static_rows"))
    dbs = [m.device_batch(b) for b in batches]
    losses = []
    for s in range(4 if graphs else STEPS):
        kw = dict(weight=WEIGHTS[s % 4]) if weights else {}
        if sample0:
            kw["sample0"] = sample0
        if static and ahead >= 2:
            kw["after_next"] = dbs[(s + 2) % 4]
        m.train_async(dbs[s % 4], LR, next_batch=dbs[(s + 1) % 4], **kw)
        losses.append(float(m.last_loss.item()))
    if graphs:
        for i in range(4):
            m.replay(m.capture_step(dbs[i], dbs[(i + 1) % 4], LR))
            losses.append(float(m.last_loss.item()))
    m.check_static_overflow()
    return digest(losses, m.gather_params(), m.gather_slots())


def worker(rank, world, port, configs, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = []
        for name, over, ctor, opts in configs:
            out.append((name, run_one(rank, world, over, ctor, **opts)))
        ret[rank] = out
    except Exception:
        import traceback
        ret[rank] = "FAIL: " + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ok = True
    for world, configs in ((1, ONE_RANK), (2, TWO_RANKS)):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        ret = ctx.Manager().dict()
        procs = [ctx.Process(target=worker, args=(r, world, port, configs, ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        if any(p.is_alive() for p in procs):      # a hang: end the children and start nothing more
            for p in procs:
                p.kill()
            print("world %d: timed out" % world)
            return 1
        for r in range(world):
            if not isinstance(ret.get(r), list):
                ok = False
                print("rank %d of %d: %s" % (r, world, ret.get(r)))
        if isinstance(ret.get(0), list):
            for name, d in ret[0]:
                print("%-34s %s" % (name, d), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

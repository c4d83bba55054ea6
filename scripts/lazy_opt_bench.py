#!/usr/bin/env python3
"""Train-step time of the lazy optimizers against lazy-L2 SGD and the dense optimizer (single GPU, resident batches):
python scripts/lazy_opt_bench.py shape=bench|10m|c5 opt=sgd|adam|lazy_adam|rmsprop|lazy_rmsprop|lazy_adagrad|lazy_rowwise_adagrad|... [steps=N] [td=bf16]
  bench: the Electronics bench shape (40 k users / 22 k items / 673 categories, d = 128, Ls = 10, B = 4096)
  10m:   10 M users / 5 M items / 10 k categories, d = 128, Ls = 10, B = 4096 (BASELINE.json's synthetic tables)
  c5:    the same tables at d = 256, Ls = 90, B = 4096
sgd runs the lazy-L2 step; the dense optimizers sweep every row of the four tables every step.  One process per
(shape, optimizer): the tables, their slots and the step's state are made on the device (init="device").
  sharded=1: the same step on a one-rank ShardedModel (tlsan_amd/dist.py, the step whose exchange sizes follow the batch,
             plan of the next batch queued a step ahead): lazy_* with the owners' lazy optimizer update
             (tlsan_shard_apply_lazy_opt), the dense names with the owners' sweep, sgd with the lazy-L2 owner update."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tlsan_amd import synth
from tlsan_amd.model import Model
kw = dict(a.split("=") for a in sys.argv[1:])
shape, opt = kw.get("shape", "bench"), kw.get("opt", "lazy_adam")
SHAPES = {"bench": dict(d=128, Ls=10, U=39991, I=22048, C=673),
          "10m": dict(d=128, Ls=10, U=10_000_000, I=5_000_000, C=10_000),
          "c5": dict(d=256, Ls=90, U=10_000_000, I=5_000_000, C=10_000)}
s = SHAPES[shape]
d, Ls, B = s["d"], s["Ls"], int(kw.get("B", 4096))
cfg = synth.make_config("electronics", Ls=Ls, hidden_units=d, itemid_embedding_size=d // 2, userid_embedding_size=d // 2,
                        cateid_embedding_size=d // 2, user_count=s["U"], item_count=s["I"], cate_count=s["C"], optimizer=opt)
lr = 1.0 if opt == "sgd" else 1e-3
icl = synth.item_cate_list(cfg)
W = int(kw.get("warmup", 5))
N = int(kw.get("steps", 50))
if kw.get("sharded", "0") == "1":
    import torch.distributed as dist
    from tlsan_amd.dist import ShardedModel
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29549")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    m = ShardedModel(cfg, icl, l2_mode="lazy" if (opt == "sgd" or opt.startswith("lazy_")) else "dense", init="device")
    dbs = [m.device_batch(b) for b in synth.make_batches(cfg, 4, B, seed=1234)]
    sstep = lambda k: m.train_async(dbs[k % 4], lr, next_batch=dbs[(k + 1) % 4])
    for k in range(W):
        sstep(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(W, W + N):
        sstep(k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / N
    print("sharded=1 shape=%s opt=%s d=%d Ls=%d B=%d shard %.2f GB: %.1f us/step over %d steps, loss %.4f"
          % (shape, opt, d, Ls, B, m.shard.numel() * 4 / 1e9, dt * 1e6, N, float(m.last_loss.item())), flush=True)
    dist.destroy_process_group()
    sys.exit(0)
m = Model(cfg, icl, l2_mode="lazy" if opt == "sgd" else "dense", table_dtype=kw.get("td", "f32"),
          init="device")
host = synth.make_batches(cfg, 4, B, seed=1234)
dbs = [m.device_batch(b) for b in host]
table_bytes = sum(getattr(m, k).numel() * getattr(m, k).element_size() for k in ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb"))


def row_launch_bytes(b):
    """Bytes the lazy optimizers' row launch (k_update_lazy_opt) moves for batch b: per used item / user row the summed
    gradient, W, m and v read and W, m, v written (seven row widths; item_b of the candidates beside them), every category
    row's summed gradient and use count read and the used ones' W, m, v read and written, the dense parameters and their
    slots.  The Adagrad forms (k_update_lazy_adagrad) keep one accumulator: a row width less read and written, or -- row-wise
    -- one float per row and table."""
    u, i, _, hi, hin, _, sl, sln, uc = (np.asarray(x) for x in b)
    Sn = hin.shape[1] if hin.ndim == 2 else 0
    items = [i, hi[np.arange(Ls)[None, :] < sl[:, None]]]
    if Sn:
        items.append(hin[np.arange(Sn)[None, :] < sln[:, None]])
    it = np.unique(np.concatenate(items))
    nc_used = len(np.unique(np.concatenate([icl[it], uc])))
    di, dc, WU = d // 2, d // 2, (d // 2 + Ls + 3) // 4 * 4
    ni, nb, nu = len(it), len(np.unique(i)), len(np.unique(u))
    if opt == "lazy_adagrad":           # (k_update_lazy_adagrad) one accumulator per element: five row widths
        return (ni * 5 * di * 4 + nb * 5 * 4 + nu * (5 * (di + Ls) + (WU - di - Ls)) * 4
                + cfg["cate_count"] * (dc + 1) * 4 + nc_used * 4 * dc * 4 + m.lay.n_dense * 6 * 4)
    if opt == "lazy_rowwise_adagrad":   # one accumulator per row: three row widths, and a float read and written per row and table
        return (ni * (3 * di + 2) * 4 + nb * 5 * 4 + nu * (3 * (di + Ls) + (WU - di - Ls) + 4) * 4
                + cfg["cate_count"] * (dc + 1) * 4 + nc_used * (2 * dc + 2) * 4 + m.lay.n_dense * 6 * 4)
    return (ni * 7 * di * 4 + nb * 7 * 4 + nu * (7 * (di + Ls) + (WU - di - Ls)) * 4
            + cfg["cate_count"] * (dc + 1) * 4 + nc_used * 6 * dc * 4 + m.lay.n_dense * 8 * 4)


def step(k):
    m.train_async(dbs[k % 4], lr, next_batch=dbs[(k + 1) % 4], after_next=dbs[(k + 2) % 4])


for k in range(W):
    step(k)
torch.cuda.synchronize()
t0 = time.perf_counter()
for k in range(W, W + N):
    step(k)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / N
print("shape=%s opt=%s d=%d Ls=%d B=%d tables %.2f GB%s: %.1f us/step, loss %.4f; lazy row launch %.1f MB/step"
      % (shape, opt, d, Ls, B, table_bytes / 1e9, " td=" + kw["td"] if "td" in kw else "", dt * 1e6, float(m._out[0].item()),
         np.mean([row_launch_bytes(b) for b in host]) / 1e6), flush=True)

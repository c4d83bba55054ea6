#!/usr/bin/env python3
"""One SHA-256 per case over what two training steps through the split lazy tail leave (k_finalize_presum, then
k_update_lazy or k_update_lazy_opt): the losses, every parameter and, under an optimizer, both slots.  For comparing two
builds of the library bit for bit -- run it once per build (TLSAN_LIB_PATH names the other one) and diff the outputs.
Cases: the smallest shapes of tests/test_gpu_lazy_opt.py::test_lazy_row_forms (U = 200, I = 300, Sn = 3; B = 24, and
B = 96 where C <= 3 so that several row-sum workgroups share a category) for d in {64, 256} (narrow and wide rows),
Ls in {10, 90} (WU > 128, Ls % 4 != 0), C in {3, 20}, fp32 and bf16 tables, lazy-L2 SGD in its split form and the three
lazy optimizers; clip 0.05, so every step is clipped.
  python scripts/lazy_rows_digest.py > digest.txt"""
import hashlib
import os
import sys

os.environ["TLSAN_LAZY_ONE_PASS"] = "0"   # (read once per process: lazy-L2 SGD takes row sums + k_update_lazy)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tests.helpers import make_config, random_batch, random_params
from tests.lazy_opt_ref import random_slots
from tlsan_amd.model import Model

CLIP = 0.05
LR = {"adam": 0.05, "rmsprop": 0.02, "adadelta": 1.0}
BF16_TABLES = ("item_emb", "user_emb", "cate_emb")
BATCH_FIELDS = ("u", "i", "y", "hist_i", "hist_i_new", "hist_t", "sl", "sl_new", "u_cate")


def digest(d, Ls, C, B, table_dtype, update, seed=80):
    lazy_opt = update != "sgd"
    cfg = make_config(U=200, I=300, C=C, d=d, Ls=Ls, regulation_rate=1e-3, max_gradient_norm=CLIP,
                      optimizer="lazy_" + update if lazy_opt else "sgd")
    p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in random_params(cfg, seed=seed).items()}
    if table_dtype == "bf16":
        for k in BF16_TABLES:
            p[k] = torch.as_tensor(p[k], dtype=torch.float32).to(torch.bfloat16).double().numpy()
    _, cat = random_batch(cfg, B=8, Sn=2, seed=seed + 2)
    m = Model(cfg, cat, l2_mode="lazy", table_dtype=table_dtype)
    m.set_params({k: np.asarray(v, np.float32) for k, v in p.items()})
    if lazy_opt:
        st = random_slots(p, update, seed + 1)
        m.set_slots([{k: np.asarray(v, np.float32) for k, v in st[s].items()} for s in ("slot1", "slot2")])
    h = hashlib.sha256()
    for s in range(2):
        b = random_batch(cfg, B=B, Sn=3, seed=seed + 10 + s)[0]
        loss = m.train(None, tuple(b[f] for f in BATCH_FIELDS), LR[update] if lazy_opt else 0.5)
        h.update(np.float64(loss).tobytes())
    got = m.get_params()
    for k in sorted(got):
        h.update(np.ascontiguousarray(got[k], np.float32).tobytes())
    for sl in m.get_slots() or []:
        for k in sorted(sl):
            h.update(np.ascontiguousarray(sl[k], np.float32).tobytes())
    torch.cuda.synchronize()
    return h.hexdigest()


if __name__ == "__main__":
    for d in (64, 256):
        for Ls in (10, 90):
            for C in (3, 20):
                for B in ((24, 96) if C <= 3 else (24,)):
                    for table_dtype in ("f32", "bf16"):
                        for update in ("sgd", "adam", "rmsprop", "adadelta"):
                            print("d=%d Ls=%d C=%d B=%d %s %s %s" % (d, Ls, C, B, table_dtype, update,
                                                                       digest(d, Ls, C, B, table_dtype, update)), flush=True)

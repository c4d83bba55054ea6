"""One sha256 per point of the evaluation side over the raw bytes of what Model.label_ranks (plain and against a seen
list), recommend, score_candidates and similar_items (both metrics) return: two libraries that print the same digests on
the same machine compute the same bits (scripts/ab.py --libs runs it once per library).  Model's own methods only, none
of the C calls (the file runs unchanged on an older checkout).  Points: d in {64, 128, 256} x f32 / bf16 tables at I = 700, B = Q = 77,
lazy L2 after two training steps (P != 1), K in {1, 16, 17, 64, 65, 100}; the gathering form (I = 270 000, d = 256: the
dense matrix would pass its cap); and integer scores that rise with the id, which overflow the append buffers."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 16, 17, 64, 65, 100)


def config(I, d, U=300, C=23):
    from tlsan_amd import synth
    return synth.make_config("electronics", user_count=U, item_count=I, cate_count=C, hidden_units=d,
                             itemid_embedding_size=d // 2, userid_embedding_size=d // 2, cateid_embedding_size=d // 2)


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, name, *tensors):
        self.h.update(name.encode())
        for t in tensors:
            a = np.ascontiguousarray(t.detach().cpu().numpy())
            self.h.update(("%s%s" % (a.dtype, a.shape)).encode())
            self.h.update(a.tobytes())

    def hex(self):
        return self.h.hexdigest()


def trained_model(cfg, table_dtype, B):
    """a lazy-L2 model with a bias on every item, two steps in: the table scale is no longer 1"""
    from tlsan_amd import synth
    from tlsan_amd.model import Model
    m = Model(cfg, synth.item_cate_list(cfg), l2_mode="lazy", table_dtype=table_dtype)
    p = m.get_params()
    p["item_b"] = np.random.RandomState(3).uniform(-0.5, 0.5, p["item_b"].shape).astype(np.float32)
    m.set_params(p)
    for b in synth.make_batches(cfg, 2, B, seed=5):
        m.train(None, b, 1.0)
    return m


def point(cfg, table_dtype, B, ks):
    from tlsan_amd import synth
    from tlsan_amd.model import SeenItems
    I, U = cfg["item_count"], cfg["user_count"]
    m = trained_model(cfg, table_dtype, B)
    tb = m.device_batch(synth.make_batches(cfg, 1, B, seed=9, test=True)[0], is_test=True)
    rng = np.random.RandomState(11)
    lens = rng.randint(0, 40, U)
    seen = SeenItems(np.concatenate([[0], np.cumsum(lens)]), np.concatenate([np.sort(rng.randint(0, I, n)) for n in lens]),
                     m.device)
    d = Digest()
    d.h.update(np.float32(m.table_scale()).tobytes())
    d.add("ranks", m.label_ranks(tb))
    d.add("ranks seen", *m.label_ranks(tb, exclude=seen, return_eligible=True))
    d.add("ranks history", m.label_ranks(tb, exclude="history"))
    d.add("candidates", m.score_candidates(tb, rng.randint(-1, I, (B, 37)).astype(np.int32)))
    items = rng.randint(0, I, B)
    lists = [np.sort(rng.randint(0, I, n)) for n in rng.randint(0, 30, B)]
    for k in ks:
        d.add("recommend %d" % k, *m.recommend(tb, k))
        d.add("recommend %d history" % k, *m.recommend(tb, k, exclude="history"))
        d.add("recommend %d seen" % k, *m.recommend(tb, k, exclude=seen))
        for metric in ("cosine", "dot"):
            d.add("similar %d %s" % (k, metric), *m.similar_items(items, k, metric=metric))
            d.add("similar %d %s lists" % (k, metric), *m.similar_items(items, k, metric=metric, exclude=lists))
    return d.hex()


def overflow_point():
    """scores that rise with the id: every later item beats the threshold (tests/test_gpu_similar.py)"""
    from tlsan_amd.model import Model
    I = 3001
    cfg = config(I, 64, U=8, C=3)
    m = Model(cfg, (np.arange(I) % 3).astype(np.int32))
    p = m.get_params()
    item = np.zeros((I, 32), np.float32)
    item[:, 0] = np.arange(I)
    item[0, 0] = 1
    item[:, 1] = np.arange(I) % 3 - 1
    p["item_emb"], p["cate_emb"] = item, np.zeros_like(p["cate_emb"])
    m.set_params(p)
    d = Digest()
    for k in (16, 64, 200):
        d.add("similar %d" % k, *m.similar_items(np.array([0, 1, 5, 3000]), k, metric="dot"))
    return d.hex()


def main():
    for dd in (64, 128, 256):
        for td in ("f32", "bf16"):
            print("%-34s %s" % ("d=%d %s I=700 B=77" % (dd, td), point(config(700, dd), td, 77, KS)), flush=True)
    print("%-34s %s" % ("d=256 f32 I=270000 B=64 (gather)", point(config(270000, 256), "f32", 64, (50,))), flush=True)
    print("%-34s %s" % ("rising scores (buffer overflow)", overflow_point()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""`Model`: the reference's ``TLSAN/model.py`` call surface over the HIP library.

Same constructor and methods as the reference class (model.py:13-313) so the reference's
``train.py`` loop drives it unchanged apart from the TensorFlow session object:

    Model(config, item_cate_list)
    .train(sess, batch, lr, add_summary=False) -> float     model.py:208-234
    .eval_auc(sess, batch) -> float                         model.py:237-263
    .eval_prec(sess, batch) / .eval_recall(sess, batch)     model.py:265-299
    .save(sess) / .restore(sess, path)                      model.py:302-313
    .global_step / .global_epoch_step / .global_epoch_step_op  (objects with .eval())
    .prec_1 ... .prec_50, .recall_1 ... .recall_50             (objects with .eval())
    .train_writer / .eval_writer                               (objects with .add_summary())

``sess`` is accepted and ignored (the reference passes a tf.Session).  ``batch`` is the 9-tuple
of ``input.py``.  All arithmetic runs in libtlsan_hip.so on the GPU; torch is used only to own
device memory and the stream.  There is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

from . import _lib as L

KS = (1, 10, 20, 30, 40, 50)  # model.py:144-156


class _Var:
    """Stand-in for the tf.Variable / tensor handles train.py calls .eval() on."""

    def __init__(self, getter):
        self._get = getter

    def eval(self, session=None):  # noqa: A003 - name fixed by the reference
        return self._get()


class _Writer:
    """tf.summary.FileWriter stand-in (model.py:18-19; train.py:91-118): scalar summaries as rows
    `step,tag,value` appended to <logdir>/scalars.csv (histogram summaries of model.py:174-181 are kept
    as their count / min / max / mean / std).  Also keeps the rows in memory (`.rows`)."""

    def __init__(self, path):
        self.path = path
        self.rows = []
        self._pending = []

    def add_summary(self, summary=None, global_step=None):
        self.rows.append((global_step, summary))
        items = summary if isinstance(summary, list) else [summary]
        for it in items:
            if isinstance(it, tuple) and len(it) == 2:
                self._pending.append((global_step, it[0], it[1]))
        if len(self._pending) >= 64:
            self.flush()

    def flush(self):
        if not self._pending:
            return
        os.makedirs(self.path, exist_ok=True)
        with open(os.path.join(self.path, "scalars.csv"), "a") as f:
            for step, tag, val in self._pending:
                f.write("%s,%s,%.9g\n" % ("" if step is None else int(step), tag, float(val)))
        self._pending = []


def glorot_uniform(rng, shape):
    """TF-1.x default initializer of tf.get_variable (model.py:62-64,70-72,79-81,446)."""
    limit = np.sqrt(6.0 / (shape[0] + shape[1]))
    return rng.uniform(-limit, limit, size=shape).astype(np.float32)


DENSE_KEYS = ("fwa1_W1", "fwa1_b1", "fwa1_W2", "fwa1_b2", "dense_K", "dense_b",
              "fwa2_W1", "fwa2_b1", "fwa2_W2", "fwa2_b2", "gamma")
TABLE_KEYS = ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb")


def dense_slices(lay, d, heads):
    """The layout of the flat `dense` vector, stated once: (name, offset, shape) of every DENSE_KEYS weight under the
    library's DenseLayout `lay` (tlsan_dense_layout_of) for hidden_units d and `heads` heads."""
    dh = d // heads
    return (("fwa1_W1", lay.f1_W1, (dh, dh)), ("fwa1_b1", lay.f1_b1, (dh,)),
            ("fwa1_W2", lay.f1_W2, (dh, dh)), ("fwa1_b2", lay.f1_b2, (dh,)),
            ("dense_K", lay.K, (d, d)), ("dense_b", lay.k0, (d,)),
            ("fwa2_W1", lay.f2_W1, (dh, dh)), ("fwa2_b1", lay.f2_b1, (dh,)),
            ("fwa2_W2", lay.f2_W2, (dh, dh)), ("fwa2_b2", lay.f2_b2, (dh,)),
            ("gamma", lay.gamma, ()))


def pack_dense(lay, d, heads, p):
    """Dict of dense weights (numpy, names as DENSE_KEYS) -> the flat [lay.n_dense] float32 vector (padding zero)."""
    out = np.zeros(lay.n_dense, np.float32)
    for k, off, shape in dense_slices(lay, d, heads):
        n = int(np.prod(shape)) if shape else 1
        out[off:off + n] = np.asarray(p[k], np.float32).reshape(-1)
    return out


def unpack_dense(lay, d, heads, flat):
    """The flat dense vector (numpy) -> dict of copies of its weights, shaped as the parameters."""
    flat = np.asarray(flat)
    out = {}
    for k, off, shape in dense_slices(lay, d, heads):
        n = int(np.prod(shape)) if shape else 1
        out[k] = flat[off:off + n].reshape(shape).copy()
    return out


def write_checkpoint(path, step, epoch, params, slots=None):
    """The single-file checkpoint TLSAN-<step>.npz: the two counters, every parameter under its name and, when the
    optimizer has accumulators (a list of dicts named like the parameters: two, or the Adagrad forms' one), those as
    slot1/<name>, slot2/<name> -- tf.train.Saver keeps the optimizer's slot variables too."""
    extra = {}
    for n, sl in enumerate(slots or (), 1):
        extra.update({"slot%d/%s" % (n, k): v for k, v in sl.items()})
    np.savez(path, global_step=step, global_epoch_step=epoch, **params, **extra)


def read_checkpoint(path, want_slots=True):
    """write_checkpoint's file -> (step, epoch, params, slots); slots lists as many slot sets as the file holds, None
    when it holds none (an sgd run) or want_slots is false."""
    z = np.load(path)
    keys = TABLE_KEYS + DENSE_KEYS
    slots = None
    if want_slots and "slot1/item_emb" in z.files:
        slots, n = [], 1
        while "slot%d/item_emb" % n in z.files:
            slots.append({k: z["slot%d/%s" % (n, k)] for k in keys})
            n += 1
    return int(z["global_step"]), int(z["global_epoch_step"]), {k: z[k] for k in keys}, slots
# optimizer -> (TLSAN_OPT_*, beta1 | decay | rho, beta2 | momentum, epsilon): TF 1.8's constructor
# defaults, which model.py:188-193 keeps (only learning_rate is passed)
OPTIMIZERS = {"sgd": (L.OPT_SGD, 0.0, 0.0, 0.0), "adam": (L.OPT_ADAM, 0.9, 0.999, 1e-8),
              "rmsprop": (L.OPT_RMSPROP, 0.9, 0.0, 1e-10), "adadelta": (L.OPT_ADADELTA, 0.95, 0.0, 1e-8)}
# the lazy ("sparse") forms: the same optimizers restricted to the rows a batch used (TLSAN_OPT_LAZY, include/tlsan.h)
LAZY_OPTIMIZERS = ("lazy_adam", "lazy_rmsprop", "lazy_adadelta")
OPTIMIZERS.update({"lazy_adam": (L.OPT_ADAM | L.OPT_LAZY, 0.9, 0.999, 1e-8),
                   "lazy_rmsprop": (L.OPT_RMSPROP | L.OPT_LAZY, 0.9, 0.0, 1e-10),
                   "lazy_adadelta": (L.OPT_ADADELTA | L.OPT_LAZY, 0.95, 0.0, 1e-8)})
# lazy Adagrad (TF's AdagradOptimizer restricted to the used rows) and row-wise Adagrad (one accumulator per table row, the
# default of DLRM / FBGEMM / TorchRec): ONE slot set, no constants but the accumulators' initial value (include/tlsan.h)
LAZY_ADAGRAD_OPTIMIZERS = ("lazy_adagrad", "lazy_rowwise_adagrad")
OPTIMIZERS.update({"lazy_adagrad": (L.OPT_ADAGRAD | L.OPT_LAZY, 0.0, 0.0, 0.0),
                   "lazy_rowwise_adagrad": (L.OPT_ROWWISE_ADAGRAD | L.OPT_LAZY, 0.0, 0.0, 0.0)})
ADAGRAD_INITIAL_ACCUMULATOR = 0.1    # TF 1.8's initial_accumulator_value
ROW_SLOT_KEYS = ("item_emb", "user_emb", "usert_emb", "cate_emb")   # lazy_rowwise_adagrad: [rows] accumulators


_STREAM_CACHE = {}
_STARTED_WORDS = []   # pinned words that kernels of queued steps write (Model._started): never freed


def concurrent_streams(device, want=1, pool=6, **stream_kw):
    """`want` new streams whose work can run WHILE the current stream is busy, and while each other is.

    HIP multiplexes streams onto a few hardware queues (four by default), round-robin over every stream the process
    has used -- torch's, RCCL's, ours.  Two streams that land on one queue execute in launch order like a single
    stream: a "side" stream that shares the main stream's queue overlaps nothing (measured on the sharded step, one
    rank: 143 us with the plan streams colliding with the main stream, 122 with one of them, 107 with neither).
    Which queue a new stream gets cannot be asked for, but it can be observed: a spin kernel on stream a, a tiny kernel
    launched after it on stream b -- b finishes early exactly when the two are on different queues."""
    dev = torch.device(device)
    main = torch.cuda.current_stream(dev)
    # one set per (device, current stream) and process: every new stream is one more tenant of the four queues, and a
    # process that builds several models (bench.py's variants) would end up with side streams sharing queues again
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), main.cuda_stream, tuple(sorted(stream_kw.items())))
    have = _STREAM_CACHE.setdefault(key, [])
    if len(have) >= want:       # (bench.py's third model, with streams of its own: 98-113 us/step instead of 57)
        return have[:want]
    cands = [torch.cuda.Stream(dev, **stream_kw) for _ in range(max(pool, want))]
    x = torch.zeros(64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def overlaps(a, b):
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(a):
            ev[0].record(a)
            torch.cuda._sleep(400000)
            ev[1].record(a)
        with torch.cuda.stream(b):
            x.add_(1.0)
            ev[2].record(b)
        torch.cuda.synchronize(dev)
        return ev[0].elapsed_time(ev[2]) < 0.5 * ev[0].elapsed_time(ev[1])

    for c in cands:                     # (a queue exists from the first use of its stream)
        with torch.cuda.stream(c):
            x.add_(1.0)
    chosen = []
    for c in cands:
        if len(chosen) < want:
            if overlaps(main, c) and all(overlaps(o, c) for o in chosen):
                chosen.append(c)
    for c in cands:                     # fewer independent queues than asked for: take what there is
        if len(chosen) < want and c not in chosen:
            chosen.append(c)
    torch.cuda.synchronize(dev)
    have[:] = chosen
    return chosen


class SeenItems:
    """Every user's seen items (input.seen_items_csr) on the device: the fourth form of `exclude` that exclusion_csr
    -- and so recommend, sample_negatives, sampled_ranks and label_ranks, single and sharded -- takes.  A row b then
    keeps out the seen list of its user db.u[b] UNITED with the row's own input (what "history" gives: a test row's
    input is not always inside its user's training list)."""

    def __init__(self, off, ids, device):
        off, ids = np.asarray(off, np.int64), np.asarray(ids, np.int64)
        if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != len(ids) or (np.diff(off) < 0).any():
            raise ValueError("SeenItems: off must be a CSR offset array [n_users + 1] over ids")
        if len(ids) and (ids.min() < 0 or ids.max() > np.iinfo(np.int32).max):
            raise ValueError("SeenItems: item ids must be non-negative int32")
        self.n_users = len(off) - 1
        self.max_len = int(np.diff(off).max())
        self.off = torch.as_tensor(off).to(device)
        self.ids = torch.as_tensor(np.concatenate([ids, [0]]).astype(np.int32)).to(device)   # (+1: never empty)

    @classmethod
    def from_train_set(cls, train_set, n_users, device):
        from .input import seen_items_csr
        return cls(*seen_items_csr(train_set, n_users), device=device)

    def rows(self, u, pad):
        """[B, max_len] int32: the list of each row's user, left-aligned, the rest `pad` (a user id outside
        0 .. n_users - 1 has an empty list: checking it would be a host round trip per batch)."""
        u = u.long()
        known = (u >= 0) & (u < self.n_users)
        u = torch.where(known, u, 0)
        lo = self.off[u]
        n = torch.where(known, self.off[u + 1] - lo, 0)
        ar = torch.arange(max(self.max_len, 1), device=u.device)[None, :]
        ok = ar < n[:, None]
        return torch.where(ok, self.ids[torch.where(ok, lo[:, None] + ar, 0)], pad).to(torch.int32)


class ItemScope:
    """A set of GLOBAL item ids held on the device, sorted and unique: the `within=` of recommend and similar_items,
    single and sharded ("the best k within these items": in stock, this region, this department).  Built from exactly
    one of items= (a sequence, array or tensor of ids, in any order, repeats allowed), mask= (bool [item_count]) or
    categories= (category ids) with item_cate= (the model's item -> category map, [item_count]).  An id outside
    [0, item_count) or a wrong shape is a ValueError; an empty scope is allowed (every list comes back -1 / -inf).
    Only the scope's items are scored: a list costs what a table of `count` items costs."""

    def __init__(self, item_count, device, items=None, mask=None, categories=None, item_cate=None):
        if (items is not None) + (mask is not None) + (categories is not None) != 1:
            raise ValueError("ItemScope: give exactly one of items=, mask= and categories=")
        host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        I = int(item_count)
        if items is not None:
            ids = host(items)
            if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
                raise ValueError("ItemScope: items must be a 1-D sequence of item ids, got shape %s dtype %s" % (ids.shape, ids.dtype))
            ids = np.unique(ids.astype(np.int64))
            if ids.size and (ids[0] < 0 or ids[-1] >= I):
                raise ValueError("ItemScope: item ids must be in [0, %d)" % I)
        elif mask is not None:
            m = host(mask)
            if m.shape != (I,) or m.dtype != np.bool_:
                raise ValueError("ItemScope: mask must be bool [%d], got shape %s dtype %s" % (I, m.shape, m.dtype))
            ids = np.flatnonzero(m).astype(np.int64)
        else:
            if item_cate is None:
                raise ValueError("ItemScope: categories= needs item_cate=, the model's item -> category map")
            ic, want = host(item_cate), host(categories)
            if ic.shape != (I,):
                raise ValueError("ItemScope: item_cate must be [%d], got shape %s" % (I, ic.shape))
            if want.ndim != 1 or (want.size and want.dtype.kind not in "iu"):
                raise ValueError("ItemScope: categories must be a 1-D sequence of category ids")
            ids = np.flatnonzero(np.isin(ic, want)).astype(np.int64)
        self.item_count, self.device = I, device
        self.count = int(ids.size)
        self._host = ids
        self.ids = torch.as_tensor(ids.astype(np.int32)).to(device)
        self._local = {}

    def local(self, id_mul, id_add, n_local):
        """The ascending LOCAL indices of the scope's items that a table of n_local items with global ids
        n * id_mul + id_add holds (a whole table: (1, 0, item_count); the item shard of rank r of W: (W, r, its count))
        -> int32 device tensor; cached per table."""
        buf, n = self.sub(id_mul, id_add, n_local)
        return buf[:n]

    def sub(self, id_mul, id_add, n_local):
        """local() as tlsan_eval_topk_scoped takes it: (buffer, nsub) -- the indices are buffer[:nsub]; the buffer is one
        element longer, so that an empty list still has an address."""
        key = (int(id_mul), int(id_add), int(n_local))
        if key not in self._local:
            rel = self._host - key[1]
            loc = rel[(rel >= 0) & (rel % key[0] == 0)] // key[0]
            loc = loc[loc < key[2]]
            self._local[key] = (torch.as_tensor(np.concatenate([loc, [0]]).astype(np.int32)).to(self.device), len(loc))
        return self._local[key]


class ItemBoost:
    """A per-item score adjustment held on the device: fp32 [item_count], one value per GLOBAL item id -- the `boost=` of
    recommend, single and sharded, reusable across calls.  A row's score of item g becomes fl(s + boost[g]), or
    fl(s + fl(boost_weight[b] * boost[g])) with row weights, INSIDE the selection (tlsan_eval_topk_scoped_boost /
    tlsan_eval_topk_lists_boost), so an item just outside the unboosted list that the boost lifts in is found.  -inf buries
    an item behind every finite score without removing it (exclude= / within= remove items); NaN ranks last.
    Built from an array or tensor of item_count values, or by of_items (a few ids against a base value) / of_categories
    (a value per category, gathered through the item -> category map); a + b adds two holders over the same items in fp32.
    device None: the tensor's own, "cpu" for an array; device "cpu" works for building and adding."""

    def __init__(self, values, device=None):
        t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
        if t.dim() != 1 or t.numel() < 1 or not (t.dtype.is_floating_point or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
            raise ValueError("ItemBoost: want a 1-D array of item_count numbers, got shape %s dtype %s" % (tuple(t.shape), t.dtype))
        self.values = t.detach().to(device=t.device if device is None else device, dtype=torch.float32).contiguous()
        self.item_count, self.device = int(t.numel()), self.values.device

    @classmethod
    def of_items(cls, item_count, ids, values, base=0.0, device="cpu"):
        """boost[ids[j]] = values[j] (values: one number for all, or one per id; an id named twice keeps its last value),
        `base` everywhere else.  An id outside [0, item_count) or a wrong shape is a ValueError."""
        host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        I, ids = int(item_count), host(ids)
        if I < 1 or ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise ValueError("ItemBoost.of_items: want item_count >= 1 and a 1-D sequence of item ids")
        if ids.size and (ids.min() < 0 or ids.max() >= I):
            raise ValueError("ItemBoost.of_items: item ids must be in [0, %d)" % I)
        vals = host(values).astype(np.float32)
        if vals.ndim != 0 and vals.shape != ids.shape:
            raise ValueError("ItemBoost.of_items: values must be one number or one per id, got shape %s for %d ids" % (vals.shape, ids.size))
        out = np.full(I, base, np.float32)
        out[ids.astype(np.int64)] = vals
        return cls(out, device=device)

    @classmethod
    def of_categories(cls, cate_values, item_cate, device=None):
        """boost[i] = cate_values[item_cate[i]]: a gather on item_cate's device (device None) or on `device`.  A category
        id outside [0, len(cate_values)) or a wrong shape is a ValueError."""
        ic = item_cate if isinstance(item_cate, torch.Tensor) else torch.as_tensor(np.asarray(item_cate))
        cv = cate_values if isinstance(cate_values, torch.Tensor) else torch.as_tensor(np.asarray(cate_values))
        if ic.dim() != 1 or ic.numel() < 1 or ic.dtype.is_floating_point or ic.dtype == torch.bool or cv.dim() != 1 or cv.numel() < 1:
            raise ValueError("ItemBoost.of_categories: want cate_values [cate_count] and item_cate [item_count] category ids")
        if int(ic.min()) < 0 or int(ic.max()) >= cv.numel():
            raise ValueError("ItemBoost.of_categories: category ids must be in [0, %d)" % cv.numel())
        dev = ic.device if device is None else device
        return cls(cv.to(device=dev, dtype=torch.float32)[ic.to(dev).long()], device=dev)

    def __add__(self, other):
        if not isinstance(other, ItemBoost):
            return NotImplemented
        if other.item_count != self.item_count:
            raise ValueError("ItemBoost: adding boosts over %d and %d items" % (self.item_count, other.item_count))
        return ItemBoost(self.values + other.values.to(self.device))


def item_boost_for(item_count, device, item_cate, values, items, categories, base):
    """Model.item_boost / ShardedModel.item_boost: fills in the count and the device (item_cate: a callable giving the
    item -> category map on the device)."""
    if (values is not None) + (items is not None) + (categories is not None) != 1:
        raise ValueError("item_boost: give exactly one of values, items=(ids, values) and categories=")
    if values is not None:
        boost = ItemBoost(values, device=device)
        if boost.item_count != item_count:
            raise ValueError("item_boost: want %d values, got %d" % (item_count, boost.item_count))
        return boost
    if items is not None:
        ids, vals = items
        return ItemBoost.of_items(item_count, ids, vals, base=base, device=device)
    return ItemBoost.of_categories(categories, item_cate(), device=device)


def boost_of(boost, boost_weight, B, item_count, device):
    """Checks recommend's `boost=` (an ItemBoost, or an array or tensor that is wrapped) and `boost_weight=` ([B] numbers,
    array or tensor) -> None without a boost, else (values [item_count] float32, weights [B] float32 or None) on `device`.
    A weight without a boost, a boost over another item count or a weight of the wrong length is a ValueError."""
    if boost is None:
        if boost_weight is not None:
            raise ValueError("boost_weight= weighs boost=: give boost=")
        return None
    if not isinstance(boost, ItemBoost):
        boost = ItemBoost(boost, device=device)
    if boost.item_count != item_count:
        raise ValueError("boost must cover the model's %d items, got %d" % (item_count, boost.item_count))
    w = None
    if boost_weight is not None:
        w = boost_weight if isinstance(boost_weight, torch.Tensor) else torch.as_tensor(np.asarray(boost_weight))
        if tuple(w.shape) != (B,) or w.dtype == torch.bool or w.dtype.is_complex:
            raise ValueError("boost_weight: want [%d] numbers, got shape %s dtype %s" % (B, tuple(w.shape), w.dtype))
        w = w.detach().to(device=device, dtype=torch.float32).contiguous()
    return boost.values.to(device), w


class ListCursor:
    """A position in each row's ranking, held on the device: ids [B] int32 and scores [B] float32 -- the `after=` of
    recommend and audience, single and sharded.  A row with ids[b] >= 0 gets the next entries of the same call's ranking
    strictly behind (scores[b], ids[b]) in the lists' order (higher score first, equal -> lower id, +0 == -0, NaN last);
    ids[b] == ListCursor.START (-2) is no cursor: the row is the call's without after=; any other negative id (-1: what a
    short page ends in) is an exhausted row, whose page is all -1 / -inf.  ListCursor.of(ids, scores) is the cursor behind
    a page (its last column, cloned), so pages chained through it tile the exact ranking at any depth, one scan a page.
    The cursor is a position, not an item: it need not be in the table, the scope or eligible.  It is a SNAPSHOT, like
    UserVectors: pages tile only while the parameters, boost, scope and exclusions stay the same; nothing detects a
    change.  device None: the tensors' own, "cpu" for arrays; device "cpu" works for building."""

    START = L.AFTER_START

    def __init__(self, ids, scores, device=None):
        i = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores))
        ints = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
        if i.dim() != 1 or i.numel() < 1 or i.dtype not in ints:
            raise ValueError("ListCursor: ids must be a 1-D array of integers, got shape %s dtype %s" % (tuple(i.shape), i.dtype))
        if s.shape != i.shape or not (s.dtype.is_floating_point or s.dtype in ints):
            raise ValueError("ListCursor: scores must be [%d] numbers, got shape %s dtype %s" % (i.numel(), tuple(s.shape), s.dtype))
        if i.dtype == torch.int64 and (int(i.min()) < -(1 << 31) or int(i.max()) >= (1 << 31)):
            raise ValueError("ListCursor: ids must fit int32")
        dev = i.device if device is None else device
        self.ids = i.detach().to(device=dev, dtype=torch.int32).contiguous()
        self.scores = s.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.device = self.ids.device

    @classmethod
    def of(cls, ids, scores):
        """The cursor behind a page (ids, scores) [B, K], as a list call returned it: its last column, cloned."""
        if not isinstance(ids, torch.Tensor) or not isinstance(scores, torch.Tensor) or ids.dim() != 2 or ids.shape != scores.shape \
                or ids.shape[1] < 1:
            raise ValueError("ListCursor.of: want a page (ids, scores) of [B, K] tensors")
        return cls(ids[:, -1].clone(), scores[:, -1].clone())

    @classmethod
    def start(cls, B, device="cpu"):
        """B rows without a cursor: after=ListCursor.start(B, device) is the call without after=, ids and bits."""
        if int(B) < 1:
            raise ValueError("ListCursor.start: want B >= 1")
        return cls(torch.full((int(B),), cls.START, dtype=torch.int32, device=device),
                   torch.zeros(int(B), dtype=torch.float32, device=device))

    def __len__(self):
        return int(self.ids.shape[0])

    @property
    def done(self):
        """[B] bool: the rows whose last page ended short (their next page is empty)."""
        return self.ids == -1

    def rows(self, rows):
        """The cursor of the rows `rows` (an index tensor) alone."""
        return ListCursor(self.ids[rows], self.scores[rows])


def cursor_of(after, B, device):
    """Checks an `after=` argument (a ListCursor, or an (ids, scores) pair of arrays or tensors that is wrapped) -> None
    without one, else the ListCursor on `device`.  Anything else, or a cursor of another length than the call's B rows, is
    a ValueError."""
    if after is None:
        return None
    if not isinstance(after, ListCursor):
        if not isinstance(after, (tuple, list)) or len(after) != 2:
            raise ValueError("after: want a ListCursor or an (ids, scores) pair, got %s" % type(after).__name__)
        try:
            after = ListCursor(after[0], after[1])
        except (TypeError, RuntimeError) as e:
            raise ValueError("after: %s" % e)
    if len(after) != B:
        raise ValueError("after: a cursor of %d rows for %d rows" % (len(after), B))
    try:
        return ListCursor(after.ids, after.scores, device=device)
    except RuntimeError as e:
        raise ValueError("after: cannot be moved to %s: %s" % (device, e))


def check_deep(n, page):
    """Checks the n and page of recommend_deep / audience_deep -> them as ints: n >= 1, page in 1..256."""
    for name, v in (("n", n), ("page", page)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, got %r" % (name, v))
    if int(n) < 1 or not 1 <= int(page) <= L.TOPK_MAX:
        raise ValueError("want n >= 1 and page in 1..%d, got n %d, page %d" % (L.TOPK_MAX, n, page))
    return int(n), int(page)


def deep_pages(topk, n, page, after=None):
    """The first n entries of a ranking in ceil(n / page) pages: topk(k, cursor) gives the k entries behind a ListCursor
    (None: the head of the list), and every page's cursor is the last column of the page before, taken on the device --
    no host read between the pages (a CategoryIndex call reads its unrestricted rows once, on the first page).  The last page asks only for what is left of n.  -> (ids [B, n], scores [B, n])."""
    ids, scores = [], []
    for p0 in range(0, n, page):
        pid, psc = topk(min(page, n - p0), after)
        ids.append(pid)
        scores.append(psc)
        if p0 + page < n:
            after = ListCursor.of(pid, psc)
    return (ids[0], scores[0]) if len(ids) == 1 else (torch.cat(ids, 1), torch.cat(scores, 1))


class CategoryIndex:
    """The items by category: a partition of the GLOBAL item ids -- of all item_count of them, or of an ItemScope's when
    within= is given -- into one list per category, held on the device: list_off [cate_count + 1] int32 and list_items
    int32, ascending by (category, id); max_list, the longest list's length, stays on the host.  The `index=` of
    recommend and similar_items, single and sharded (Model.category_index / ShardedModel.category_index build it): a
    row that asks for a category scores that category's list and nothing else.  A category without items is an empty
    list; an index over an empty scope is allowed (every list is empty).  item_cate: [item_count] category ids in
    [0, cate_count) (array or tensor); device "cpu" works.  The index is a snapshot of item_cate: rebuild it when the
    map changes."""

    PROBES = 8    # LISTS_PMAX (csrc/tlsan_lists.h): most lists a row probes

    def __init__(self, item_cate, cate_count, device, within=None):
        ic = item_cate.detach().cpu().numpy() if isinstance(item_cate, torch.Tensor) else np.asarray(item_cate)
        I, C = int(ic.shape[0]) if ic.ndim == 1 else -1, int(cate_count)
        if I < 0 or C < 1 or ic.dtype.kind not in "iu" or (I and (ic.min() < 0 or ic.max() >= C)):
            raise ValueError("CategoryIndex: item_cate must be a 1-D array of category ids in [0, %d)" % C)
        if within is not None and (not isinstance(within, ItemScope) or within.item_count != I):
            raise ValueError("CategoryIndex: within must be None or an ItemScope over the %d items" % I)
        ids = np.arange(I, dtype=np.int64) if within is None else within._host
        cat = ic[ids].astype(np.int64)
        order = np.argsort(cat, kind="stable")                 # (ids ascend, so a stable sort keeps them ascending in a list)
        self.item_count, self.cate_count, self.device, self.within = I, C, device, within
        self._items, self._cats = ids[order], cat[order]
        self.count = int(ids.size)
        off = np.concatenate([[0], np.cumsum(np.bincount(self._cats, minlength=C))])
        self.max_list = int(np.diff(off).max())
        self.list_off = torch.as_tensor(off.astype(np.int32)).to(device)
        self.list_items = torch.as_tensor(self._items.astype(np.int32)).to(device)
        self._local = {}
        self._lens, self._plans = {}, {}    # per table: the lists' lengths (host); per (table, thresholds): the shelves' plan

    def local(self, id_mul, id_add, n_local):
        """The index of a table of n_local items whose local item n is global id n * id_mul + id_add (a whole table:
        (1, 0, item_count); the item shard of rank r of W: (W, r, its count)) -> (list_off [cate_count + 1] int32,
        list_items int32 LOCAL indices ascending by (category, index) -- one element longer than the lists, so that an
        empty index still has an address -- and the longest list's length); cached per table."""
        key = (int(id_mul), int(id_add), int(n_local))
        if key not in self._local:
            rel = self._items - key[1]
            keep = (rel >= 0) & (rel % key[0] == 0) & (rel // key[0] < key[2])
            off = np.concatenate([[0], np.cumsum(np.bincount(self._cats[keep], minlength=self.cate_count))])
            items = np.concatenate([rel[keep] // key[0], [0]])
            self._lens[key] = np.diff(off)
            self._local[key] = (torch.as_tensor(off.astype(np.int32)).to(self.device),
                                torch.as_tensor(items.astype(np.int32)).to(self.device), int(np.diff(off).max()))
        return self._local[key]

    def shelf_plan(self, id_mul, id_add, n_local, seg_items, big_items):
        """The ShelfPlan of local()'s index of that table under the two thresholds (shelves_plan), built from the host copy
        of the lists' lengths; cached per (table, thresholds)."""
        key = (int(id_mul), int(id_add), int(n_local))
        self.local(*key)
        pk = key + (int(seg_items), int(big_items))
        if pk not in self._plans:
            self._plans[pk] = ShelfPlan(self._lens[key], seg_items, big_items, self.device)
        return self._plans[pk]


def index_of(index, item_count, cate_count):
    """Checks an `index=` argument -> it (None: no index)."""
    if index is not None and (not isinstance(index, CategoryIndex) or index.item_count != item_count or index.cate_count != cate_count):
        raise ValueError("index must be None or a CategoryIndex over the model's %d items in %d categories" % (item_count, cate_count))
    return index


def recommend_index(index, within, item_count, cate_count):
    """Checks recommend's `index=` -> it (None: no index): the scope belongs to the index, so it goes without within=."""
    index = index_of(index, item_count, cate_count)
    if index is not None and within is not None:
        raise ValueError("within= and index= together: the scope belongs to the index, category_index(within=scope)")
    return index


def similar_index(index, within, same_category, item_count, cate_count):
    """Checks similar_items' `index=` -> it (None: no index): it goes with same_category=True and without within=."""
    index = index_of(index, item_count, cate_count)
    if index is not None and not same_category:
        raise ValueError("index= needs same_category=True: the index is by category")
    if index is not None and within is not None:
        raise ValueError("within= and index= together: the scope belongs to the index, category_index(within=scope)")
    return index


def index_categories(category, B, cate_count, device):
    """Checks the `category=` that goes with an index ([B] or [B, P] category ids, P <= CategoryIndex.PROBES, array or
    tensor; negative: no probe, a row of negatives only is unrestricted) -> contiguous int32 [B, P] device tensor.  None,
    an id >= cate_count or a wrong shape is a ValueError."""
    if category is None:
        raise ValueError("index= needs category=: the categories each row asks for")
    cat = category if isinstance(category, torch.Tensor) else torch.as_tensor(np.asarray(category))
    shape = tuple(cat.shape)
    if shape == (B,):
        cat = cat.reshape(B, 1)
    elif len(shape) != 2 or shape[0] != B or not 1 <= shape[1] <= CategoryIndex.PROBES:
        raise ValueError("category: with an index want [%d] or [%d, P] category ids, P in 1..%d, got shape %s"
                         % (B, B, CategoryIndex.PROBES, shape))
    if cat.dtype.is_floating_point or cat.dtype == torch.bool:
        raise ValueError("category: want category ids, got dtype %s" % cat.dtype)
    if int(cat.max()) >= cate_count:
        raise ValueError("category: ids must be below %d (negative: no probe)" % cate_count)
    return cat.to(device).clamp(min=-1).to(torch.int32).contiguous()


def lists_topk(lib, dims, cparams, ut, B, k, excl, lists, row_lists, id_mul, id_add, workspace, stream, boost=None, after=None):
    """tlsan_eval_topk_lists on u_t [B, d]: the k best of the union of the lists row_lists [B, P] int32 names, of the index
    `lists` (CategoryIndex.local's triple) -> (ids [B, k] int32, scores [B, k] float32).  boost: boost_of's pair (values by
    GLOBAL id, the B rows' weights or None) -> tlsan_eval_topk_lists_boost, the scores adjusted inside the selection.
    after: the B rows' ListCursor -> tlsan_eval_topk_lists_after, with the boost or without."""
    k, P = int(k), int(row_lists.shape[1])
    off, items, max_list = lists
    nl = int(off.shape[0]) - 1
    nws = lib.tlsan_lists_workspace_bytes(C.byref(dims), B, P, k, nl, max_list)
    if nws == 0:
        raise L.TlsanError("tlsan_lists_workspace_bytes: %s" % lib.tlsan_last_error().decode())
    ws = workspace(nws)
    ids = torch.empty(B, k, dtype=torch.int32, device=ut.device)
    scores = torch.empty(B, k, dtype=torch.float32, device=ut.device)
    xoff, xid = excl
    ptr = lambda t: None if t is None else t.data_ptr()
    args = (C.byref(dims), C.byref(cparams), ut.data_ptr(), B, k, ptr(xoff), ptr(xid), off.data_ptr(), items.data_ptr(), nl,
            max_list, row_lists.data_ptr(), P, id_mul, id_add, ids.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    if after is not None:
        bp = (None, None) if boost is None else (boost[0].data_ptr(), ptr(boost[1]))
        L.check(lib.tlsan_eval_topk_lists_after(*args, *bp, after.ids.data_ptr(), after.scores.data_ptr()), "tlsan_eval_topk_lists_after")
    elif boost is None:
        L.check(lib.tlsan_eval_topk_lists(*args), "tlsan_eval_topk_lists")
    else:
        L.check(lib.tlsan_eval_topk_lists_boost(*args, boost[0].data_ptr(), ptr(boost[1])), "tlsan_eval_topk_lists_boost")
    return ids, scores


def lists_similar_topk(lib, dims, cparams, vec, inv, qids, k, metric, excl, lists, row_lists, id_mul, id_add, workspace, stream):
    """tlsan_similar_topk_lists: similar_topk over the lists row_lists [Q, P] int32 names, of the index `lists`
    (CategoryIndex.local's triple), SIMILAR_CHUNK queries at a time."""
    Q, k, P = int(qids.shape[0]), int(k), int(row_lists.shape[1])
    off, items, max_list = lists
    nl = int(off.shape[0]) - 1
    ids = torch.empty(Q, k, dtype=torch.int32, device=qids.device)
    scores = torch.empty(Q, k, dtype=torch.float32, device=qids.device)
    xoff, xid = excl
    for q0 in range(0, Q, SIMILAR_CHUNK):
        n = min(SIMILAR_CHUNK, Q - q0)
        nws = lib.tlsan_lists_workspace_bytes(C.byref(dims), n, P, k, nl, max_list)
        if nws == 0:
            raise L.TlsanError("tlsan_lists_workspace_bytes: %s" % lib.tlsan_last_error().decode())
        ws = workspace(nws)
        # (a chunk's rows keep their offsets into the one id array: the offsets are absolute)
        L.check(lib.tlsan_similar_topk_lists(C.byref(dims), C.byref(cparams), vec[q0:].data_ptr(), inv[q0:].data_ptr(),
                                             qids[q0:].data_ptr(), n, k, metric, None if xoff is None else xoff[q0:].data_ptr(),
                                             None if xid is None else xid.data_ptr(), off.data_ptr(), items.data_ptr(), nl,
                                             max_list, row_lists[q0:].data_ptr(), P, id_mul, id_add, ids[q0:].data_ptr(),
                                             scores[q0:].data_ptr(), ws.data_ptr(), ws.numel(), stream),
                "tlsan_similar_topk_lists")
    return ids, scores


def excl_rows(excl, rows, B):
    """The exclusion CSR (exclusion_csr's: every row a slot of the same width) of the rows `rows` of B alone."""
    off, xid = excl
    if off is None:
        return excl
    w = xid.numel() // B
    vals = xid.view(B, w)[rows].contiguous()
    return torch.arange(0, (vals.shape[0] + 1) * w, w, dtype=torch.int32, device=xid.device), vals.view(-1)


def indexed_topk(lib, dims, cparams, ut, B, k, excl, index, row_lists, id_mul, id_add, n_local, workspace, stream, boost=None,
                 after=None, found=None):
    """recommend's lists with an index on u_t [B, d]: the rows that probe a list go through lists_topk; the rows whose
    entries are all negative are unrestricted -- they run through the path without an index (scoped_topk over the index's
    scope, eval_topk without one) as a sub-batch and are scattered back.  One host read says whether there are any.
    boost (boost_of's pair): the sub-batch carries the boost and its rows' slice of the weights.  after (the B rows'
    ListCursor): the sub-batch carries its rows' cursors the same way, through scoped_topk.  found: a dict kept by a caller
    that pages (recommend_deep): the unrestricted rows are the same on every page, so the first call leaves them in it and
    the later ones read nothing from the device."""
    ids, scores = lists_topk(lib, dims, cparams, ut, B, k, excl, index.local(id_mul, id_add, n_local), row_lists, id_mul, id_add,
                             workspace, stream, boost=boost, after=after)
    if found is None or "free" not in found:
        free = torch.nonzero((row_lists < 0).all(1))[:, 0]
        if found is not None:
            found["free"] = free
    free = free if found is None else found["free"]
    if free.numel():
        sub_ut, sub_excl, n = ut[free].contiguous(), excl_rows(excl, free, B), int(free.numel())
        sub_boost = None if boost is None else (boost[0], None if boost[1] is None else boost[1][free].contiguous())
        if index.within is None and boost is None and after is None:
            fid, fsc = eval_topk(lib, dims, cparams, sub_ut, n, k, sub_excl, id_mul, id_add, workspace, stream)
        else:
            sub = None if index.within is None else index.within.sub(id_mul, id_add, n_local)
            fid, fsc = scoped_topk(lib, dims, cparams, sub_ut, n, k, sub_excl, sub, None, id_mul, id_add, workspace, stream,
                                   boost=sub_boost, after=None if after is None else after.rows(free))
        ids[free], scores[free] = fid, fsc
    return ids, scores


SHELF_SMAX, SHELF_MMAX, SHELF_SKIP_MAX, SHELF_SLICES_MAX = 32, 64, 8, 16   # csrc/tlsan_shelves.h


def shelves_plan(lens, seg_items, big_items):
    """The plan tlsan_eval_shelves takes, from the lists' lengths lens [nlists] (host): the lists with items, in list
    order, either packed into segments of about seg_items items (a list goes into the open segment while the segment
    stays within seg_items; a segment holds at least one list) or, when longer than big_items, cut into at most
    SHELF_SLICES_MAX slices of max(seg_items, 256) positions or more (a multiple of 256).  big_items = 0: every list is big.
    -> (seg_off [nseg + 1], seg_lists [nsmall], big_off [nbig + 1], big_slices [nbs, 3]) int32 arrays.  Which plan is used
    changes the launch geometry, never the result."""
    lens = np.asarray(lens, np.int64)
    seg_items, big_items = int(seg_items), int(big_items)
    if seg_items < 1 or big_items < 0:
        raise ValueError("shelves: seg_items must be >= 1 and big_items >= 0, got %d and %d" % (seg_items, big_items))
    seg_off, seg_lists, big_off, big_slices, fill = [0], [], [0], [], 0
    for c in np.flatnonzero(lens > 0):
        n = int(lens[c])
        if n > big_items:
            sl = max(seg_items, 256, -(-n // SHELF_SLICES_MAX))
            sl = -(-sl // 256) * 256
            big_slices += [(c, lo, min(n, lo + sl)) for lo in range(0, n, sl)]
            big_off.append(len(big_slices))
            continue
        if fill and fill + n > seg_items:
            seg_off.append(len(seg_lists))
            fill = 0
        seg_lists.append(c)
        fill += n
    if fill:
        seg_off.append(len(seg_lists))
    i32 = lambda x, shape: np.asarray(x, np.int32).reshape(shape)
    return i32(seg_off, -1), i32(seg_lists, -1), i32(big_off, -1), i32(big_slices, (-1, 3))


def shelves_thresholds(total, B):
    """The production (seg_items, big_items) of an index of `total` items for B rows (profiles/shelves.md): about
    2048 / ceil(B / 16) units, a power of two in 32..1024, so that the grid (row tiles, units) fills the device a few
    times over while the [B, units, S, m] workspace stays small; a list is big from four segments' worth."""
    tiles = (int(B) + 15) // 16
    units = 1 << int(np.log2(min(1024, max(32, 2048 // tiles))))
    seg = -(-max(1024, -(-int(total) // units)) // 256) * 256
    return seg, 4 * seg


class ShelfPlan:
    """shelves_plan's arrays on the device (each one element longer than its content, so that an empty one still has an
    address) with their host counts."""

    def __init__(self, lens, seg_items, big_items, device):
        so, sl, bo, bs = shelves_plan(lens, seg_items, big_items)
        self.nseg, self.nsmall, self.nbig, self.nbs = len(so) - 1, len(sl), len(bo) - 1, len(bs)
        dev = lambda x: torch.as_tensor(np.concatenate([x.reshape(-1), [0]]).astype(np.int32)).to(device)
        self.seg_off, self.seg_lists, self.big_off, self.big_slices = dev(so), dev(sl), dev(bo), dev(bs)


def shelves_sizes(S, m, min_items, rank_at):
    """Checks the four sizes of a page of shelves -> them as ints.  1 <= S <= 32, 1 <= m <= 64, S * m <= 256 (TOPK_MAX, the
    width list_metrics takes), 1 <= min_items <= m, 0 <= rank_at < min_items; anything else is a ValueError."""
    vals = []
    for name, v in (("shelves", S), ("k", m), ("min_items", min_items), ("rank_at", rank_at)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("shelves: %s must be an integer, got %r" % (name, v))
        vals.append(int(v))
    S, m, min_items, rank_at = vals
    if not 1 <= S <= SHELF_SMAX:
        raise ValueError("shelves: shelves must be in 1..%d, got %d" % (SHELF_SMAX, S))
    if not 1 <= m <= SHELF_MMAX:
        raise ValueError("shelves: k must be in 1..%d, got %d" % (SHELF_MMAX, m))
    if S * m > L.TOPK_MAX:
        raise ValueError("shelves: shelves * k must be at most %d, got %d * %d" % (L.TOPK_MAX, S, m))
    if not 1 <= min_items <= m:
        raise ValueError("shelves: min_items must be in 1..k = %d, got %d" % (m, min_items))
    if not 0 <= rank_at < min_items:
        raise ValueError("shelves: rank_at must be in 0..min_items - 1 = %d, got %d" % (min_items - 1, rank_at))
    return S, m, min_items, rank_at


def shelves_index(index, item_count, cate_count):
    """Checks shelves' `index=` -> it: a CategoryIndex over the model's items and categories, required."""
    if not isinstance(index, CategoryIndex) or index.item_count != item_count or index.cate_count != cate_count:
        raise ValueError("shelves: index must be a CategoryIndex over the model's %d items in %d categories (category_index())"
                         % (item_count, cate_count))
    return index


def shelves_skip(skip, B, cate_count, device):
    """Checks shelves' `skip=` (None, [B] or [B, X] category ids, X <= 8, array or tensor; negative: nothing) ->
    contiguous int32 [B, X] device tensor, or None.  An id >= cate_count or a wrong shape is a ValueError."""
    if skip is None:
        return None
    sk = skip if isinstance(skip, torch.Tensor) else torch.as_tensor(np.asarray(skip))
    shape = tuple(sk.shape)
    if shape == (B,):
        sk = sk.reshape(B, 1)
    elif len(shape) != 2 or shape[0] != B or not 1 <= shape[1] <= SHELF_SKIP_MAX:
        raise ValueError("shelves: skip must be [%d] or [%d, X] category ids, X in 1..%d, got shape %s" % (B, B, SHELF_SKIP_MAX, shape))
    if sk.dtype.is_floating_point or sk.dtype == torch.bool or sk.dtype.is_complex:
        raise ValueError("shelves: skip must hold category ids, got dtype %s" % sk.dtype)
    if int(sk.max()) >= cate_count:
        raise ValueError("shelves: skip ids must be below %d (negative: nothing is skipped)" % cate_count)
    return sk.to(device).clamp(min=-1).to(torch.int32).contiguous()


def shelves_topk(lib, dims, cparams, ut, B, S, m, min_items, rank_at, excl, lists, skip, id_mul, id_add, workspace, stream,
                 seg_items=None, big_items=None, plan=None):
    """tlsan_eval_shelves on u_t [B, d]: each row's S best lists of the index `lists` (CategoryIndex.local's triple; any
    lists of local items serve) with their m best items -> (cats [B, S] int32, ids [B, S, m] int32, scores [B, S, m]
    float32).  skip: shelves_skip's tensor or None.  plan: a ShelfPlan of the index (CategoryIndex.shelf_plan caches them);
    None: built here from the offsets, which are read back from the device -- for callers with lists of their own.
    seg_items / big_items: the plan's thresholds, None: shelves_thresholds' production values; they decide the launch
    geometry and never the result."""
    off, items, max_list = lists
    nl = int(off.shape[0]) - 1
    if plan is None:
        lens = np.diff(off.detach().cpu().numpy().astype(np.int64))
        dflt = shelves_thresholds(int(lens.clip(min=0).sum()), B)
        plan = ShelfPlan(lens, dflt[0] if seg_items is None else seg_items, dflt[1] if big_items is None else big_items, ut.device)
    nws = lib.tlsan_shelves_workspace_bytes(C.byref(dims), B, S, m, plan.nseg, plan.nbig, plan.nbs)
    if nws == 0:
        raise L.TlsanError("tlsan_shelves_workspace_bytes: %s" % lib.tlsan_last_error().decode())
    ws = workspace(nws)
    cats = torch.empty(B, S, dtype=torch.int32, device=ut.device)
    ids = torch.empty(B, S, m, dtype=torch.int32, device=ut.device)
    scores = torch.empty(B, S, m, dtype=torch.float32, device=ut.device)
    xoff, xid = excl
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(lib.tlsan_eval_shelves(C.byref(dims), C.byref(cparams), ut.data_ptr(), B, S, m, min_items, rank_at, ptr(xoff), ptr(xid),
                                   off.data_ptr(), items.data_ptr(), nl, max_list, plan.seg_off.data_ptr(),
                                   plan.seg_lists.data_ptr(), plan.nseg, plan.nsmall, plan.big_off.data_ptr(),
                                   plan.big_slices.data_ptr(), plan.nbig, plan.nbs, ptr(skip), 0 if skip is None else int(skip.shape[1]),
                                   id_mul, id_add, cats.data_ptr(), ids.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel(),
                                   stream), "tlsan_eval_shelves")
    return cats, ids, scores


def last_items(db):
    """The last item of each row's input, on the device -> [B] int64: hist_i_new[b, sl_new[b] - 1] when the row has a
    current session, else hist_i[b, sl[b] - 1], else -1 (no input)."""
    last = lambda h, n: h.long().gather(1, (n - 1).clamp(min=0)[:, None])[:, 0]
    sl = db.sl.long()
    item = torch.where(sl > 0, last(db.hist_i, sl), -1)
    if db.Sn > 0:
        sn = db.sl_new.long()
        item = torch.where(sn > 0, last(db.hist_i_new.reshape(db.B, db.Sn), sn), item)
    return item


def last_item_categories(db, item_cate):
    """The category of the last item of each row's input (last_items), on the device -> [B] int32; -1 for a row without
    input (any category).  The `category=` of "more from the department you are in".  db: a DeviceBatch
    (Model.device_batch); item_cate: the model's [item_count] device map."""
    item = last_items(db)
    return torch.where(item >= 0, item_cate.long()[item.clamp(min=0)], -1).to(torch.int32)


def batch_rows(batch):
    """The number of rows of a batch as the models take it: the reference's tuple or a DeviceBatch."""
    return batch.B if isinstance(batch, DeviceBatch) else len(batch[0])


def scope_within(within, item_count):
    """Checks a `within=` argument -> it (None: no scope)."""
    if within is not None and (not isinstance(within, ItemScope) or within.item_count != item_count):
        raise ValueError("within must be None or an ItemScope over the model's %d items" % item_count)
    return within


def scope_categories(category, B, cate_count, device):
    """Checks a `category=` argument ([B] category ids, array or tensor; negative: the row is unrestricted) -> contiguous
    int32 device tensor, or None.  An id >= cate_count or a wrong shape is a ValueError."""
    if category is None:
        return None
    cat = category if isinstance(category, torch.Tensor) else torch.as_tensor(np.asarray(category))   # (an array: checked on the host)
    if tuple(cat.shape) != (B,) or cat.dtype.is_floating_point or cat.dtype == torch.bool:
        raise ValueError("category: want [%d] category ids, got shape %s dtype %s" % (B, tuple(cat.shape), cat.dtype))
    if int(cat.max()) >= cate_count:
        raise ValueError("category: ids must be below %d (negative: the row is unrestricted)" % cate_count)
    return cat.to(device).clamp(min=-1).to(torch.int32).contiguous()


def scoped_topk(lib, dims, cparams, ut, B, k, excl, sub, row_cate, id_mul, id_add, workspace, stream, boost=None, after=None):
    """tlsan_eval_topk_scoped on u_t [B, d]: eval_topk over the local items sub (ItemScope.sub's pair; None: every item)
    with the rows' wanted categories row_cate ([B] int32 or None) -> (ids [B, k] int32, scores [B, k] float32).  boost:
    boost_of's pair (values by GLOBAL id, the B rows' weights or None) -> tlsan_eval_topk_scoped_boost, the scores adjusted
    inside the selection.  after: the B rows' ListCursor -> tlsan_eval_topk_scoped_after, with the boost or without."""
    k = int(k)
    sub, nsub = (None, -1) if sub is None else sub
    nws = lib.tlsan_scope_workspace_bytes(C.byref(dims), B, k, nsub)
    if nws == 0:
        raise L.TlsanError("tlsan_scope_workspace_bytes: %s" % lib.tlsan_last_error().decode())
    ws = workspace(nws)
    ids = torch.empty(B, k, dtype=torch.int32, device=ut.device)
    scores = torch.empty(B, k, dtype=torch.float32, device=ut.device)
    off, xid = excl
    ptr = lambda t: None if t is None else t.data_ptr()
    args = (C.byref(dims), C.byref(cparams), ut.data_ptr(), B, k, ptr(off), ptr(xid), ptr(sub), nsub, ptr(row_cate), id_mul, id_add,
            ids.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    if after is not None:
        bp = (None, None) if boost is None else (boost[0].data_ptr(), ptr(boost[1]))
        L.check(lib.tlsan_eval_topk_scoped_after(*args, *bp, after.ids.data_ptr(), after.scores.data_ptr()), "tlsan_eval_topk_scoped_after")
    elif boost is None:
        L.check(lib.tlsan_eval_topk_scoped(*args), "tlsan_eval_topk_scoped")
    else:
        L.check(lib.tlsan_eval_topk_scoped_boost(*args, boost[0].data_ptr(), ptr(boost[1])), "tlsan_eval_topk_scoped_boost")
    return ids, scores


def scoped_similar_topk(lib, dims, cparams, vec, inv, qids, k, metric, excl, sub, row_cate, id_mul, id_add, workspace, stream):
    """tlsan_similar_topk_scoped: similar_topk over the local items sub (ItemScope.sub's pair; None: every item) with the queries' wanted
    categories row_cate ([Q] int32 or None), SIMILAR_CHUNK queries at a time."""
    Q, k = int(qids.shape[0]), int(k)
    sub, nsub = (None, -1) if sub is None else sub
    ids = torch.empty(Q, k, dtype=torch.int32, device=qids.device)
    scores = torch.empty(Q, k, dtype=torch.float32, device=qids.device)
    off, xid = excl
    ptr = lambda t: None if t is None else t.data_ptr()
    for q0 in range(0, Q, SIMILAR_CHUNK):
        n = min(SIMILAR_CHUNK, Q - q0)
        nws = lib.tlsan_scope_workspace_bytes(C.byref(dims), n, k, nsub)
        if nws == 0:
            raise L.TlsanError("tlsan_scope_workspace_bytes: %s" % lib.tlsan_last_error().decode())
        ws = workspace(nws)
        # (a chunk's rows keep their offsets into the one id array: the offsets are absolute)
        L.check(lib.tlsan_similar_topk_scoped(C.byref(dims), C.byref(cparams), vec[q0:].data_ptr(), inv[q0:].data_ptr(),
                                              qids[q0:].data_ptr(), n, k, metric, None if off is None else off[q0:].data_ptr(),
                                              ptr(xid), ptr(sub), nsub, None if row_cate is None else row_cate[q0:].data_ptr(),
                                              id_mul, id_add, ids[q0:].data_ptr(), scores[q0:].data_ptr(), ws.data_ptr(),
                                              ws.numel(), stream), "tlsan_similar_topk_scoped")
    return ids, scores


def _input_items(db, pad):
    """[B, Ls + Sn] int32: the items the row's input holds (hist_i[b, :sl[b]], hist_i_new[b, :sl_new[b]]), the rest
    `pad` (the padding past the lengths is item 0, a real item, so the lengths decide)."""
    B, dev = db.B, db.i.device
    ar = torch.arange(db.hist_i.shape[1], device=dev)[None, :]
    vals = [torch.where(ar < db.sl.long()[:, None], db.hist_i, pad)]
    if db.Sn > 0:
        ar = torch.arange(db.Sn, device=dev)[None, :]
        vals.append(torch.where(ar < db.sl_new.long()[:, None], db.hist_i_new.reshape(B, db.Sn), pad))
    return torch.cat(vals, 1).to(torch.int32)


def exclusion_csr(db, exclude, n_items):
    """Per-row item lists to keep out of a recommendation, as the CSR tlsan_eval_topk takes: (excl_off [B + 1],
    excl_ids) int32 device tensors.  exclude: None -> (None, None); "history" -> the items the row's input holds,
    hist_i[b, :sl[b]] and hist_i_new[b, :sl_new[b]] (the padding past the lengths is item 0, a real item, so the
    lengths decide); a sequence of B arrays of item ids; or a SeenItems holder -> the seen list of the row's user
    db.u[b] united with the row's own input.  Built on the device without a host round trip: every row
    is a slot of the same width, sorted, its repeats and its unused slots set to INT32_MAX (ids outside the table are
    ignored by the kernel, so they sort to the end of the row and cost nothing)."""
    if exclude is None:
        return None, None
    B, dev, pad = db.B, db.i.device, np.iinfo(np.int32).max
    if isinstance(exclude, SeenItems):
        vals = torch.cat([exclude.rows(db.u, pad), _input_items(db, pad)], 1)
    elif isinstance(exclude, str):
        if exclude != "history":
            raise ValueError("exclude must be None, 'history', a SeenItems or a sequence of per-row id arrays")
        vals = _input_items(db, pad)
    else:
        vals = _listed_items(exclude, B, n_items, dev, pad)
    return _csr_of_slots(vals, pad)


def _listed_items(exclude, B, n_items, dev, pad):
    """A sequence of B arrays of item ids -> [B, widest] int32 device tensor, the rest (and ids outside the table) `pad`."""
    if len(exclude) != B:
        raise ValueError("exclude: %d lists for %d rows" % (len(exclude), B))
    lists = [np.asarray(x, np.int64).reshape(-1) for x in exclude]
    host = np.full((B, max([len(x) for x in lists] + [1])), pad, np.int64)
    for r, x in enumerate(lists):
        host[r, :len(x)] = x
    host[(host < 0) | (host >= n_items)] = pad
    return torch.as_tensor(host.astype(np.int32)).to(dev)


def _csr_of_slots(vals, pad):
    """[B, w] item ids (unused slots `pad`) -> the CSR of exclusion_csr: every row sorted, its repeats set to `pad`."""
    B, dev = vals.shape[0], vals.device
    vals = torch.sort(vals, 1).values
    vals[:, 1:] = torch.where(vals[:, 1:] == vals[:, :-1], pad, vals[:, 1:])    # repeats
    vals = torch.sort(vals, 1).values.contiguous()
    off = torch.arange(0, (B + 1) * vals.shape[1], vals.shape[1], dtype=torch.int32, device=dev)
    return off, vals.view(-1)


def grow_workspace(owner, name, nbytes, factor=1.0):
    """The grow-only uint8 device workspace kept as `owner.<name>`, with room for nbytes: allocated anew, nbytes * factor
    large, only when there is none or it is too small."""
    buf = getattr(owner, name, None)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * factor), dtype=torch.uint8, device=owner.device)
        setattr(owner, name, buf)
    return buf


def eval_topk(lib, dims, cparams, ut, B, k, excl, id_mul, id_add, workspace, stream):
    """tlsan_eval_topk on u_t [B, d] -> (ids [B, k] int32, scores [B, k] float32) device tensors.
    workspace(nbytes) returns a uint8 device tensor of at least nbytes."""
    k = int(k)
    nws = lib.tlsan_topk_workspace_bytes(C.byref(dims), B, k)
    if nws == 0:
        raise L.TlsanError("tlsan_topk_workspace_bytes: %s" % lib.tlsan_last_error().decode())
    ws = workspace(nws)
    ids = torch.empty(B, k, dtype=torch.int32, device=ut.device)
    scores = torch.empty(B, k, dtype=torch.float32, device=ut.device)
    off, xid = excl
    L.check(lib.tlsan_eval_topk(C.byref(dims), C.byref(cparams), ut.data_ptr(), B, k,
                                None if off is None else off.data_ptr(), None if xid is None else xid.data_ptr(),
                                id_mul, id_add, ids.data_ptr(), scores.data_ptr(), ws.data_ptr(), ws.numel(), stream),
            "tlsan_eval_topk")
    return ids, scores


RERANK_STAGING = 256 << 20   # bytes: no staging buffer of a diversified recommend is larger (k_all_emb's rule)


def rerank_pool(k, diversity, per_category, pool):
    """Checks recommend's diversity arguments -> the pool size N of the re-ranking stage, or None when none is asked for
    (diversity == 0 and per_category == 0: the plain top-k path).  N = pool, or min(256, max(4 k, 32))."""
    k, per_category = int(k), int(per_category)
    diversity = float(diversity)
    if not 0.0 <= diversity <= 1.0:   # (a NaN fails)
        raise ValueError("diversity must be in [0, 1], got %r" % (diversity,))
    if per_category < 0:
        raise ValueError("per_category must be >= 0, got %d" % per_category)
    if diversity == 0.0 and per_category == 0:
        if pool is not None:
            raise ValueError("pool is the candidate pool of a diversified list: give diversity or per_category with it")
        return None
    N = int(pool) if pool is not None else min(L.RERANK_MAX, max(4 * k, 32))
    if not 1 <= k <= N <= L.RERANK_MAX:
        raise ValueError("want 1 <= k <= pool <= %d, got k %d, pool %d" % (L.RERANK_MAX, k, N))
    return N


def rerank_chunk(N, d, copies=1):
    """Rows of a diversified recommend handled at a time: `copies` staged [rows * N, d] float32 matrices stay within
    RERANK_STAGING bytes."""
    return max(1, RERANK_STAGING // (copies * N * d * 4))


def rerank(lib, pool_ids, pool_scores, vec, inv, cate, k, diversity, per_category, ids, scores, stream):
    """tlsan_rerank on the pools [B, N] with their entries' vectors [B * N, d], inverse norms and categories [B * N]
    -> written into ids [B, k] int32 and scores [B, k] float32 (contiguous device tensors)."""
    B, N = pool_ids.shape
    L.check(lib.tlsan_rerank(pool_ids.data_ptr(), pool_scores.data_ptr(), vec.data_ptr(), inv.data_ptr(), cate.data_ptr(),
                             B, N, int(vec.shape[1]), int(k), float(diversity), int(per_category), ids.data_ptr(),
                             scores.data_ptr(), stream), "tlsan_rerank")


ListMetrics = collections.namedtuple("ListMetrics", "n pair_cos ild n_cate max_cate hit_pos weight_sum")
ListMetrics.__doc__ = """Per-row measurements of lists (tlsan_list_metrics), [B] device tensors: n valid entries (int32),
pair_cos the summed pairwise cosines (float64), ild = 1 - pair_cos / (n (n - 1) / 2) (float64, NaN where n < 2, not
clamped), n_cate distinct categories, max_cate the most entries sharing one, hit_pos the label's position or -1 (int32),
weight_sum the summed entry weights (float64)."""


def list_metric_inputs(ids, labels, item_weight, exposure, item_count, device):
    """Checks list_metrics' arguments (ValueError before any launch) -> (ids [B, K] int32, labels [B] int32 or None,
    item_weight [item_count] float32 or None) contiguous device tensors."""
    as_dev = lambda x, dt: (x.to(device=device, dtype=dt) if isinstance(x, torch.Tensor)
                            else torch.as_tensor(np.asarray(x)).to(device=device, dtype=dt)).contiguous()
    shape = tuple(ids.shape) if isinstance(ids, torch.Tensor) else np.shape(ids)
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError("ids: want a [B, K] array of item ids, got shape %s" % (shape,))
    if not 1 <= shape[1] <= L.LISTM_MAX:
        raise ValueError("ids: K must be in 1..%d, got %d" % (L.LISTM_MAX, shape[1]))
    if labels is not None:
        lshape = tuple(labels.shape) if isinstance(labels, torch.Tensor) else np.shape(labels)
        if lshape != (shape[0],):
            raise ValueError("labels: want [%d] item ids, got shape %s" % (shape[0], lshape))
    if item_weight is not None:
        wshape = tuple(item_weight.shape) if isinstance(item_weight, torch.Tensor) else np.shape(item_weight)
        if wshape != (item_count,):
            raise ValueError("item_weight: want [%d] weights, one per item, got shape %s" % (item_count, wshape))
    if exposure is not None:
        if not isinstance(exposure, torch.Tensor) or exposure.dtype != torch.int32 or tuple(exposure.shape) != (item_count,) \
                or not exposure.is_contiguous() or exposure.device.type != torch.device(device).type:
            raise ValueError("exposure: want a contiguous [%d] int32 counter on %s" % (item_count, device))
    ids = as_dev(ids, torch.int32)
    if int(ids.max()) >= item_count:
        raise ValueError("ids: item ids must be below %d (-1: no entry)" % item_count)
    return (ids, None if labels is None else as_dev(labels, torch.int32),
            None if item_weight is None else as_dev(item_weight, torch.float32))


def list_metrics(lib, ids, vec, inv, cate, labels, weight, exposure, stream):
    """tlsan_list_metrics on the lists ids [B, K] int32 with their entries' vectors [B * K, d], inverse norms and
    categories [B * K] (item_vectors' / rerank's staging), labels [B] int32 or None, weight [B * K] float32 or None and
    exposure, an int32 device counter over the items the call adds to, or None -> ListMetrics."""
    B, K = ids.shape
    dev = ids.device
    i32 = lambda: torch.empty(B, dtype=torch.int32, device=dev)
    f64 = lambda: torch.empty(B, dtype=torch.float64, device=dev)
    n, n_cate, max_cate, hit_pos, pair_cos, weight_sum = i32(), i32(), i32(), i32(), f64(), f64()
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(lib.tlsan_list_metrics(ids.data_ptr(), vec.data_ptr(), inv.data_ptr(), cate.data_ptr(), ptr(labels), ptr(weight),
                                   B, K, int(vec.shape[1]), n.data_ptr(), pair_cos.data_ptr(), n_cate.data_ptr(),
                                   max_cate.data_ptr(), hit_pos.data_ptr(), weight_sum.data_ptr(), ptr(exposure),
                                   0 if exposure is None else int(exposure.shape[0]), stream), "tlsan_list_metrics")
    nd = n.to(torch.float64)
    ild = 1.0 - pair_cos / (nd * (nd - 1.0) * 0.5)      # (n < 2: pair_cos is exactly 0 and so is the count of pairs -- 0 / 0, NaN)
    return ListMetrics(n, pair_cos, ild, n_cate, max_cate, hit_pos, weight_sum)


def list_metrics_chunks(ids, labels, rows, measure):
    """ListMetrics of the lists ids [B, K], `rows` of them at a time (rerank_chunk: no staged matrix beyond
    RERANK_STAGING): measure(ids_chunk, labels_chunk) -> ListMetrics of a chunk; the chunks' rows concatenated."""
    parts = [measure(ids[r0:r0 + rows], None if labels is None else labels[r0:r0 + rows])
             for r0 in range(0, int(ids.shape[0]), rows)]
    return parts[0] if len(parts) == 1 else ListMetrics(*[torch.cat(f) for f in zip(*parts)])


SIMILAR_METRICS = {"dot": L.SIM_DOT, "cosine": L.SIM_COSINE}
SIMILAR_CHUNK = 4096   # queries per tlsan_similar_topk call: bounds the slices' lists in the workspace (Q x slices x K)


def similar_queries(items, item_count, metric, exclude, device):
    """Checks similar_items' arguments -> (ids [Q] int32 device tensor, metric constant, exclusion CSR)."""
    if metric not in SIMILAR_METRICS:
        raise ValueError("metric must be 'cosine' or 'dot', got %r" % (metric,))
    host = items.detach().cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
    if host.ndim != 1 or host.size < 1 or host.dtype.kind not in "iu":
        raise ValueError("items: want a 1-D sequence of item ids, got shape %s dtype %s" % (host.shape, host.dtype))
    host = host.astype(np.int64)
    if host.min() < 0 or host.max() >= item_count:
        raise ValueError("items: ids must be in [0, %d)" % item_count)
    pad = np.iinfo(np.int32).max
    excl = (None, None) if exclude is None else _csr_of_slots(_listed_items(exclude, len(host), item_count, device, pad), pad)
    return torch.as_tensor(host.astype(np.int32)).to(device), SIMILAR_METRICS[metric], excl


def item_vectors(lib, dims, cparams, qids, id_mul, id_add, stream):
    """tlsan_item_vectors for the global ids qids [Q] int32 -> (vec [Q, d] float32, inv [Q] float32): the stored vectors
    and inverse norms of the ids this table holds, zeros for the others."""
    Q = int(qids.shape[0])
    vec = torch.empty(Q, dims.d, dtype=torch.float32, device=qids.device)
    inv = torch.empty(Q, dtype=torch.float32, device=qids.device)
    L.check(lib.tlsan_item_vectors(C.byref(dims), C.byref(cparams), qids.data_ptr(), Q, id_mul, id_add, vec.data_ptr(),
                                   inv.data_ptr(), stream), "tlsan_item_vectors")
    return vec, inv


def similar_topk(lib, dims, cparams, vec, inv, qids, k, metric, excl, id_mul, id_add, workspace, stream):
    """tlsan_similar_topk over the queries (vec, inv, qids), SIMILAR_CHUNK at a time -> (ids [Q, k] int32, scores [Q, k]
    float32) device tensors.  workspace(nbytes) returns a uint8 device tensor of at least nbytes."""
    Q, k = int(qids.shape[0]), int(k)
    ids = torch.empty(Q, k, dtype=torch.int32, device=qids.device)
    scores = torch.empty(Q, k, dtype=torch.float32, device=qids.device)
    off, xid = excl
    for q0 in range(0, Q, SIMILAR_CHUNK):
        n = min(SIMILAR_CHUNK, Q - q0)
        nws = lib.tlsan_similar_workspace_bytes(C.byref(dims), n, k)
        if nws == 0:
            raise L.TlsanError("tlsan_similar_workspace_bytes: %s" % lib.tlsan_last_error().decode())
        ws = workspace(nws)
        # (a chunk's rows keep their offsets into the one id array: the offsets are absolute)
        L.check(lib.tlsan_similar_topk(C.byref(dims), C.byref(cparams), vec[q0:].data_ptr(), inv[q0:].data_ptr(),
                                       qids[q0:].data_ptr(), n, k, metric,
                                       None if off is None else off[q0:].data_ptr(), None if xid is None else xid.data_ptr(),
                                       id_mul, id_add, ids[q0:].data_ptr(), scores[q0:].data_ptr(), ws.data_ptr(),
                                       ws.numel(), stream), "tlsan_similar_topk")
    return ids, scores


def topk_merge(lib, cand_ids, cand_scores, stream):
    """tlsan_topk_merge: [B, n_lists, k] sorted lists of disjoint items -> (ids [B, k], scores [B, k])."""
    B, n, k = cand_ids.shape
    ids = torch.empty(B, k, dtype=torch.int32, device=cand_ids.device)
    scores = torch.empty(B, k, dtype=torch.float32, device=cand_ids.device)
    L.check(lib.tlsan_topk_merge(cand_ids.contiguous().data_ptr(), cand_scores.contiguous().data_ptr(), B, n, k,
                                 ids.data_ptr(), scores.data_ptr(), stream), "tlsan_topk_merge")
    return ids, scores


AUDIENCE_CHUNK = 4096   # queries per tlsan_dense_topk call: bounds the slices' lists in the workspace (Q x slices x K)


class UserVectors:
    """The rows' representations u_t as a reusable object -- what Model.user_vectors / ShardedModel.user_vectors return and
    audience takes: vec [N, d] float32 and user [N] int32 (the batch's u) on the device.  A row is a SAMPLE: a user at a point of
    their history.  row0 / n_total: the global number of row 0 and the number of rows over all holders (0 and N on a Model;
    on a ShardedModel the ranks' rows follow each other in rank order).  A snapshot of the model `owner` at its global
    step `step`: audience refuses it once the model has trained on, like the indexes it is rebuilt after training."""

    def __init__(self, vec, user, owner, step, row0=0, n_total=None, group=None, world=1):
        self.vec, self.user = vec.contiguous(), user.to(torch.int32).contiguous()
        self.owner, self.step = owner, int(step)
        self.row0, self.n_total = int(row0), int(vec.shape[0] if n_total is None else n_total)
        self.group, self.world = group, int(world)
        self._all_users = None

    def __len__(self):
        return int(self.vec.shape[0])

    def users_of(self, rows):
        """The user ids of global row numbers (tensor or array of any shape, as audience returns them; -1 stays -1) ->
        int32 device tensor of that shape.  On a sharded model the call is collective the first time: the ranks' `user`
        arrays are gathered once and kept."""
        if self._all_users is None:
            users = self.user
            if self.world > 1:
                from .dist_comm import allgather_rows
                n = allgather_rows(torch.tensor([len(self)], device=users.device), self.group).tolist()
                padded = torch.full((max(max(n), 1),), -1, dtype=torch.int32, device=users.device)
                padded[:len(self)] = users
                got = allgather_rows(padded, self.group).view(len(n), -1)
                users = torch.cat([got[r, :n[r]] for r in range(len(n))])
            self._all_users = users
        rows = torch.as_tensor(rows).to(self._all_users.device).long()
        if self._all_users.numel() == 0:
            return torch.full_like(rows, -1, dtype=torch.int32)
        return torch.where(rows >= 0, self._all_users[rows.clamp(min=0)], -1).to(torch.int32)


def batch_list(batches):
    """user_vectors' argument -> a list of batches: one batch (a tuple of arrays or a DeviceBatch) or an iterable of them."""
    if isinstance(batches, DeviceBatch) or (isinstance(batches, tuple) and len(batches) > 0 and not
                                            isinstance(batches[0], (tuple, DeviceBatch))):
        return [batches]
    return list(batches)


def kept_rows(real, n):
    """user_vectors' real= -> how many rows of each of the n batches are kept (None: all of them)."""
    if real is None:
        return [None] * n
    real = [int(r) for r in (real if isinstance(real, (list, tuple, np.ndarray)) else [real])]
    if len(real) != n or min(real + [0]) < 0:
        raise ValueError("real: want one non-negative row count per batch (%d batches)" % n)
    return real


def audience_queries(items, k, item_count, device):
    """Checks audience's items and k -> the ids [Q] as an int32 device tensor."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= L.TOPK_MAX:
        raise ValueError("k must be an integer in 1..%d, got %r" % (L.TOPK_MAX, k))
    host = items.detach().cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)
    if host.ndim != 1 or host.size < 1 or host.dtype.kind not in "iu":
        raise ValueError("items: want a 1-D sequence of item ids, got shape %s dtype %s" % (host.shape, host.dtype))
    host = host.astype(np.int64)
    if host.min() < 0 or host.max() >= item_count:
        raise ValueError("items: ids must be in [0, %d)" % item_count)
    return torch.as_tensor(host.astype(np.int32)).to(device)


def check_user_vectors(users, owner, step, d, device):
    """audience's refusals about `users`: anything but a UserVectors of this model at its current global step."""
    if not isinstance(users, UserVectors):
        raise ValueError("users: want the UserVectors that user_vectors() returns, got %s" % type(users).__name__)
    if users.owner is not owner:
        raise ValueError("users: these UserVectors come from another model")
    if users.step != step:
        raise ValueError("users: taken at global step %d, the model is at %d -- rebuild them after training" % (users.step, step))
    have, device = users.vec.device, torch.device(device)
    other = have.type != device.type or (have.index is not None and device.index is not None and have.index != device.index)
    if users.vec.dim() != 2 or users.vec.shape[1] != d or users.vec.dtype != torch.float32 or other:
        raise ValueError("users: vec must be [N, %d] float32 on %s" % (d, device))
    if users.user.shape != users.vec.shape[:1]:
        raise ValueError("users: user must be [N]")


def seen_rows_csr(seen_off, seen_ids, user, items, row0=0):
    """The item -> rows transposition of a seen-items CSR for the query items: (off [Q + 1] int32, rows int32), query q's
    list the global numbers row0 + n, ascending, of the rows n whose user user[n] has items[q] in their seen list
    seen_ids[seen_off[u] : seen_off[u + 1]].  A user id outside the CSR has seen nothing; a repeated query item gets
    its list again.  Torch on the tensors' device (CPU tensors work), one sort of the (query item, row) pairs that hit,
    no loop over items or rows."""
    dev = user.device
    seen_off, seen_ids, items = seen_off.to(dev).long(), seen_ids.to(dev).long(), items.to(dev).long()
    n_users, N, Q = int(seen_off.shape[0]) - 1, int(user.shape[0]), int(items.shape[0])
    u = user.long()
    known = (u >= 0) & (u < n_users)
    u = torch.where(known, u, torch.zeros_like(u))
    lo = seen_off[u]
    n = torch.where(known, seen_off[u + 1] - lo, torch.zeros_like(lo))
    start = torch.cumsum(n, 0) - n
    row = torch.repeat_interleave(torch.arange(N, device=dev), n)          # the row of every (row, seen item) pair
    item = seen_ids[lo[row] + (torch.arange(int(row.shape[0]), device=dev) - start[row])]
    uq, slot_of = torch.unique(items, return_inverse=True)                # the distinct query items, ascending
    pos = torch.searchsorted(uq, item).clamp(max=int(uq.shape[0]) - 1)
    hit = uq[pos] == item
    key = torch.unique(pos[hit] * max(N, 1) + row[hit])                    # (sorted; a seen list that repeats an item counts once)
    kslot, krow = torch.div(key, max(N, 1), rounding_mode="floor"), key % max(N, 1)
    cnt = torch.bincount(kslot, minlength=int(uq.shape[0]))
    ustart = torch.cumsum(cnt, 0) - cnt
    qn = cnt[slot_of]                                                      # every query's list, repeats included
    off = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(qn, 0)
    qq = torch.repeat_interleave(torch.arange(Q, device=dev), qn)
    src = ustart[slot_of[qq]] + (torch.arange(int(qq.shape[0]), device=dev) - off[qq])
    rows = torch.cat([krow[src] + int(row0), torch.zeros(1, dtype=torch.int64, device=dev)])   # (+1: never empty)
    return off.to(torch.int32), rows.to(torch.int32)


def audience_exclusion(exclude, qids, users):
    """audience's exclude -> the CSR of global row numbers tlsan_dense_topk takes: None -> (None, None); a SeenItems ->
    seen_rows_csr over these rows (a rank's own rows are all its scan can meet); a sequence of Q sequences of global row
    numbers -> _csr_of_slots, numbers outside [0, n_total) dropped."""
    if exclude is None:
        return None, None
    if isinstance(exclude, SeenItems):
        return seen_rows_csr(exclude.off, exclude.ids[:-1], users.user, qids, users.row0)
    if isinstance(exclude, str):
        raise ValueError("exclude must be None, a SeenItems or a sequence of per-item arrays of row numbers")
    pad = np.iinfo(np.int32).max
    return _csr_of_slots(_listed_items(exclude, int(qids.shape[0]), users.n_total, qids.device, pad), pad)


def dense_topk(lib, q, x, scale, bias, excl, id_add, k, workspace, stream, after=None):
    """tlsan_dense_topk over the queries q [Q, d] against the matrix x [N, d], AUDIENCE_CHUNK queries at a time -> (ids
    [Q, k] int32, scores [Q, k] float32) device tensors.  scale / bias: [Q] float32 device tensors or None.  after: the Q
    queries' ListCursor, in global row ids -> tlsan_dense_topk_after."""
    Q, d, N, k = int(q.shape[0]), int(q.shape[1]), int(x.shape[0]), int(k)
    ids = torch.empty(Q, k, dtype=torch.int32, device=q.device)
    scores = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    off, xid = excl
    ptr = lambda t, q0=0: None if t is None else t[q0:].data_ptr()
    for q0 in range(0, Q, AUDIENCE_CHUNK):
        n = min(AUDIENCE_CHUNK, Q - q0)
        nws = lib.tlsan_dense_topk_workspace_bytes(n, N, k)
        if nws == 0:
            raise L.TlsanError("tlsan_dense_topk_workspace_bytes: %s" % lib.tlsan_last_error().decode())
        ws = workspace(nws)
        # (a chunk's queries keep their offsets into the one id array: the offsets are absolute)
        args = (q[q0:].data_ptr(), n, d, x.data_ptr(), N, ptr(scale, q0), ptr(bias, q0), ptr(off, q0), ptr(xid), id_add, k,
                ids[q0:].data_ptr(), scores[q0:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
        if after is None:
            L.check(lib.tlsan_dense_topk(*args), "tlsan_dense_topk")
        else:
            L.check(lib.tlsan_dense_topk_after(*args, after.ids[q0:].data_ptr(), after.scores[q0:].data_ptr()), "tlsan_dense_topk_after")
    return ids, scores


EXPLAIN_BY = {"position": L.EXPLAIN_BY_POSITION, "item": L.EXPLAIN_BY_ITEM}
EXPLAIN_ORDER = {"positive": L.EXPLAIN_POSITIVE, "abs": L.EXPLAIN_ABS}


def explain_args(top, by, order):
    """Checks explain's switches -> (r, by, order) as tlsan_explain takes them.  top: an integer in 1..16; by: "item" or
    "position"; order: "positive" or "abs"."""
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= int(top) <= L.EXPLAIN_RMAX:
        raise ValueError("explain: top must be an integer in 1..%d, got %r" % (L.EXPLAIN_RMAX, top))
    if by not in EXPLAIN_BY:
        raise ValueError("explain: by must be 'item' or 'position', got %r" % (by,))
    if order not in EXPLAIN_ORDER:
        raise ValueError("explain: order must be 'positive' or 'abs', got %r" % (order,))
    return int(top), EXPLAIN_BY[by], EXPLAIN_ORDER[order]


class Explanation:
    """What Model.explain returns, device tensors: parts [B, Kc, R] float32 or None (R = 3 + Ls + Sn, the columns that
    columns() names); src, item [B, Kc, top] int32 and value [B, Kc, top] float32, the strongest history sources of every
    (row, item) -- src the column of parts the source starts at, item the id it holds; -1 / -1 / 0 where a row has fewer
    sources and for padding items; kind: 0 where src is in the long window, 1 in the session, -1 where src is -1."""

    def __init__(self, parts, src, item, value, Ls):
        self.parts, self.src, self.item, self.value, self.Ls = parts, src, item, value, Ls
        self.kind = torch.where(src < 0, torch.full_like(src, -1), (src >= 3 + Ls).to(torch.int32))

    @staticmethod
    def columns(Ls, Sn):
        """The names of the R = 3 + Ls + Sn columns of parts."""
        return ["bias", "user", "bridge"] + ["long[%d]" % l for l in range(Ls)] + ["session[%d]" % j for j in range(Sn)]


def explain(lib, dims, cparams, db, att0, att1, items, r, by, order, want_parts, stream):
    """tlsan_explain on a device batch, the attention tensors of its forward and items [B, Kc] int32 -> Explanation."""
    if not hasattr(lib, "tlsan_explain"):
        raise L.TlsanError("this build of the library has no tlsan_explain")
    B, Kc = items.shape
    R = 3 + dims.Ls + db.Sn
    parts = torch.empty(B, Kc, R, dtype=torch.float32, device=items.device) if want_parts else None
    src = torch.empty(B, Kc, r, dtype=torch.int32, device=items.device)
    item = torch.empty_like(src)
    val = torch.empty(B, Kc, r, dtype=torch.float32, device=items.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    L.check(lib.tlsan_explain(C.byref(dims), C.byref(cparams), C.byref(db.c), att0.data_ptr(), att1.data_ptr(), items.data_ptr(),
                              Kc, r, by, order, ptr(parts), ptr(src), ptr(item), ptr(val), None, 0, stream), "tlsan_explain")
    return Explanation(parts, src, item, val, dims.Ls)


def candidate_tensor(candidates, B, device):
    """[B, C] global item ids (array or tensor, -1 = padding) -> contiguous int32 device tensor."""
    if isinstance(candidates, torch.Tensor):
        cand = candidates.to(device=device, dtype=torch.int32)
    else:
        cand = torch.as_tensor(np.asarray(candidates, np.int64).astype(np.int32)).to(device)
    if cand.dim() != 2 or cand.shape[0] != B or cand.shape[1] < 1:
        raise ValueError("candidates: want a [%d, C] array of item ids, got shape %s" % (B, tuple(cand.shape)))
    return cand.contiguous()


def score_candidates(lib, dims, cparams, ut, cand, id_mul, id_add, stream, scores=None):
    """tlsan_score_candidates on u_t [B, d] and cand [B, C] int32 -> scores [B, C] float32 (written into `scores` when
    given: the item-sharded form leaves the ids it does not hold untouched)."""
    B, Cn = cand.shape
    if scores is None:
        scores = torch.empty(B, Cn, dtype=torch.float32, device=cand.device)
    L.check(lib.tlsan_score_candidates(C.byref(dims), C.byref(cparams), ut.data_ptr(), B, Cn, cand.data_ptr(), id_mul,
                                       id_add, scores.data_ptr(), stream), "tlsan_score_candidates")
    return scores


def candidate_ranks(lib, cand, scores, stream):
    """tlsan_candidate_ranks: how many of each row's candidates 1.. come ahead of candidate 0 -> [B] int32."""
    B, Cn = cand.shape
    ranks = torch.empty(B, dtype=torch.int32, device=cand.device)
    L.check(lib.tlsan_candidate_ranks(cand.data_ptr(), scores.contiguous().data_ptr(), B, Cn, ranks.data_ptr(), stream),
            "tlsan_candidate_ranks")
    return ranks


def sample_negatives(lib, item_count, labels, n, seed, row0, excl, stream):
    """tlsan_sample_negatives for the rows of labels [B] int32 (global row row0 + b) -> [B, n] int32."""
    B = int(labels.shape[0])
    out = torch.empty(B, int(n), dtype=torch.int32, device=labels.device)
    off, xid = excl
    L.check(lib.tlsan_sample_negatives(int(item_count), labels.contiguous().data_ptr(), B, int(n),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), None if off is None else off.data_ptr(),
                                       None if xid is None else xid.data_ptr(), out.data_ptr(), stream),
            "tlsan_sample_negatives")
    return out


def sampled_ranks(lib, item_count, db, ut, n, seed, row0, exclude, score, stream):
    """Rank of each row's label among its n sampled negatives -> [B] int32 device tensor: one sampling, one scoring of
    [label | negatives] by score(u_t, cand) -> [B, 1 + n] scores, one ranking; no host round trip."""
    neg = sample_negatives(lib, item_count, db.i, n, seed, row0, exclusion_csr(db, exclude, item_count), stream)
    cand = torch.cat([db.i.view(-1, 1).to(torch.int32), neg], 1).contiguous()
    return candidate_ranks(lib, cand, score(ut, cand), stream)


class TopKCounters:
    """The streaming precision_at_k / recall_at_k state (model.py:265-299): hits per k of KS and rows counted, one
    pair for each metric, cumulative over every update like the reference's never-reset local variables
    (train.py:75-76,82)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.hits_p = np.zeros(len(KS), np.int64)
        self.hits_r = np.zeros(len(KS), np.int64)
        self.n_p = self.n_r = 0

    def add_prec(self, hits, n):
        """Count a batch (hits [len(KS)]: rows whose label ranks below k; n rows) -> P@k so far."""
        self.hits_p += hits
        self.n_p += n
        return [self.hits_p[i] / (k * self.n_p) for i, k in enumerate(KS)]

    def add_recall(self, hits, n):
        self.hits_r += hits
        self.n_r += n
        return [self.hits_r[i] / self.n_r for i in range(len(KS))]


def exposure_stats(exposure, n_items):
    """(coverage, gini) of an exposure counter over n_items items (array or tensor; int32 counters are read as the
    uint32 the kernel adds to): the share of items with exposure > 0, and the Gini coefficient of the exposure over ALL
    n_items items, sum_i (2 i - I - 1) x_(i) / (I sum x) over the ascending x_(1) <= ... <= x_(I) -- 0 when uniform,
    (I - 1) / I when one item takes everything, NaN when nothing was exposed."""
    x = exposure.detach().cpu().numpy() if isinstance(exposure, torch.Tensor) else np.asarray(exposure)
    n_items = int(n_items)
    x = np.sort(x.reshape(-1)[:n_items].astype(np.int64) & 0xFFFFFFFF)
    if len(x) != n_items or n_items < 1:
        raise ValueError("exposure: want a counter over %d items, got %d" % (n_items, len(x)))
    total = int(x.sum())
    if total == 0:
        return 0.0, float("nan")
    lead = int(((2 * np.arange(1, n_items + 1, dtype=np.int64) - n_items - 1) * x).sum())   # (exact: integers)
    return float(int((x > 0).sum())) / n_items, float(lead) / (float(n_items) * float(total))


class ListMetricCounters:
    """Accumulates ListMetrics of batches of lists of one length K on the device; result() makes the one host read.
    Integer quantities (rows, valid entries, categories, the histogram of hit positions) are summed exactly, the two
    double sums (ILD over the rows with n >= 2, the weights) per batch and then over the batches: the result does not
    depend on how the rows were split into batches beyond the rounding of those two sums (1e-12 relative)."""
    N_INT = 6   # rows, short rows, sum n, rows n >= 1, sum n_cate, rows n >= 2; then [K + 1] rows by hit position + 1
                # (0: no hit) and [K + 1] rows by max_cate -- counts, so that processes' states add up (reduce)

    def __init__(self):
        self.k = self._int = self._dbl = None

    def add(self, metrics, k):
        """Count a batch's ListMetrics (possibly of no rows); k: the length K of its lists (the same in every call)."""
        k, m = int(k), metrics
        if self.k is None:
            self.k = k
            self._int = torch.zeros(self.N_INT + 2 * (k + 1), dtype=torch.int64, device=m.n.device)
            self._dbl = torch.zeros(2, dtype=torch.float64, device=m.n.device)
        elif k != self.k:
            raise ValueError("ListMetricCounters: lists of length %d after lists of length %d" % (k, self.k))
        n, s, one = m.n.to(torch.int64), self._int, torch.ones_like(m.n, dtype=torch.int64)
        s[:self.N_INT] += torch.stack([one.sum(), (n < k).sum(), n.sum(), (n >= 1).sum(),
                                       m.n_cate.to(torch.int64).sum(), (n >= 2).sum()])     # (n_cate is 0 on an empty row)
        s[self.N_INT:self.N_INT + k + 1].scatter_add_(0, m.hit_pos.to(torch.int64) + 1, one)
        s[self.N_INT + k + 1:].scatter_add_(0, m.max_cate.to(torch.int64), one)
        self._dbl += torch.stack([torch.where(m.n >= 2, m.ild, torch.zeros_like(m.ild)).sum(), m.weight_sum.sum()])

    def reduce(self, total):
        """Several processes' counters into one: total(tensor) -> the exact sum of an int64 / float64 tensor over them."""
        self._int, self._dbl = total(self._int), total(self._dbl)

    def result(self, exposure=None, n_items=None):
        """-> {"ILD@K": mean ILD over the rows with n >= 2, "categories@K": mean n_cate over the rows with n >= 1,
        "max_per_category": max of max_cate over the rows, "HR@K" / "NDCG@K" / "MRR@K": from the hit positions over ALL
        rows with full_ranking_metrics' formulas (a hit at position p is worth 1, 1 / log2(p + 2), 1 / (p + 1)),
        "novelty@K": sum weight_sum / sum n, "coverage@K" / "gini@K": exposure_stats of the exposure counter (NaN
        without one), "rows", "short_rows": rows with n < K}, K the lists' length; a mean over no rows is NaN."""
        if self.k is None:
            raise ValueError("ListMetricCounters: nothing was added")
        k = self.k
        v = torch.cat([self._int, self._dbl.view(torch.int64)]).cpu().numpy()     # the one host read
        ints, dbl = v[:-2], v[-2:].copy().view(np.float64)
        rows, short, sum_n, rows1, sum_cate, rows2 = (int(x) for x in ints[:self.N_INT])
        hits = ints[self.N_INT + 1:self.N_INT + k + 1]
        by_max = np.nonzero(ints[self.N_INT + k + 1:])[0]
        p = np.arange(k, dtype=np.float64)
        ratio = lambda a, b: float(a) / b if b else float("nan")
        cov, gini = (float("nan"), float("nan")) if exposure is None else \
            exposure_stats(exposure, len(exposure) if n_items is None else n_items)
        return {"ILD@%d" % k: ratio(dbl[0], rows2), "categories@%d" % k: ratio(sum_cate, rows1),
                "max_per_category": int(by_max[-1]) if len(by_max) else 0,
                "HR@%d" % k: ratio(int(hits.sum()), rows),
                "NDCG@%d" % k: ratio(float((hits / np.log2(p + 2.0)).sum()), rows),
                "MRR@%d" % k: ratio(float((hits / (p + 1.0)).sum()), rows),
                "novelty@%d" % k: ratio(dbl[1], sum_n), "coverage@%d" % k: cov, "gini@%d" % k: gini,
                "rows": rows, "short_rows": short}


def hits_and_rows(ranks):
    """What TopKCounters counts of a batch's label ranks (array or tensor) -> [len(KS) + 1] int64 array: the rows whose
    label ranks below k for the k of KS, then the row count -- integers, so the vectors of the ranks' shares add up."""
    r = ranks.cpu().numpy() if isinstance(ranks, torch.Tensor) else np.asarray(ranks)
    return np.array([(r < k).sum() for k in KS] + [len(r)], np.int64)


SAMPLED_KS = (1, 5, 10, 20)


def rank_histogram(ranks, n):
    """[n + 1] int64 counts of the sampled ranks 0 .. n (what sampled_metrics needs: sums of counts are exact, so the
    metrics do not depend on how the rows were split into launches or ranks)."""
    r = np.asarray(ranks.cpu().numpy() if isinstance(ranks, torch.Tensor) else ranks, np.int64).reshape(-1)
    if r.size and (r.min() < 0 or r.max() > n):
        raise ValueError("sampled ranks must lie in 0..%d" % n)
    return np.bincount(r, minlength=n + 1).astype(np.int64)


def _histogram_sums(hist, ks):
    """HR@k, NDCG@k and MRR of a rank histogram (hist[r] rows of rank r), summed in float64 -- the one implementation,
    for the sampled evaluation (metrics_from_histogram) and the full ranking (full_ranking_metrics)."""
    hist = np.asarray(hist, np.int64)
    rows = int(hist.sum())
    r = np.arange(len(hist), dtype=np.float64)
    h = hist.astype(np.float64)
    out = {}
    for k in ks:
        out["HR@%d" % k] = float(hist[:k].sum()) / rows
    for k in ks:
        out["NDCG@%d" % k] = float((h[:k] / np.log2(r[:k] + 2.0)).sum()) / rows
    out["MRR"] = float((h / (r + 1.0)).sum()) / rows
    return out


def metrics_from_histogram(hist, n, ks=SAMPLED_KS):
    """The sampled-evaluation metrics of a rank histogram (rank_histogram), summed in float64:
    HR@k = mean(rank < k), NDCG@k = mean([rank < k] / log2(rank + 2)), MRR = mean(1 / (rank + 1)),
    AUC_N = mean(1 - rank / n)."""
    hist = np.asarray(hist, np.int64)
    rows = int(hist.sum())
    out = _histogram_sums(hist, ks)
    out["AUC_N"] = 1.0 - float(int((hist * np.arange(len(hist), dtype=np.int64)).sum())) / (float(n) * rows)
    return out


def full_ranking_metrics(hist, ks=SAMPLED_KS):
    """HR@k, NDCG@k and MRR of the histogram of the (filtered) label ranks over all items (rank_histogram with
    n = item_count - 1; Model.label_ranks(exclude=)).  Counts are exact integers, so histograms of launches and of ranks
    add up and the result does not depend on the split.  AUC_N is not defined here: the number of eligible items
    differs from row to row."""
    return _histogram_sums(hist, ks)


def sampled_metrics(ranks, n, ks=SAMPLED_KS):
    """HR@k, NDCG@k, MRR and AUC_N of the ranks of the labels among n sampled negatives (Model.sampled_ranks)."""
    return metrics_from_histogram(rank_histogram(ranks, n), n, ks)


class DeviceBatch:
    """The placeholders of model.py:27-53 as int32 / fp32 device tensors + the C struct."""

    def __init__(self, batch, device, is_test=False, Ls=None):
        u, i, yj, hist_i, hist_i_new, hist_t, sl, new_sl, c = batch
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(np.asarray(a)), dtype=dt).to(device, non_blocking=True)
        self.B = int(len(u))
        if self.B < 1:
            raise ValueError("empty batch")
        hist_i = np.asarray(hist_i)
        hist_i_new = np.asarray(hist_i_new).reshape(self.B, -1)
        if Ls is not None and hist_i.shape != (self.B, Ls):
            raise ValueError("hist_i must be [B, Ls=%d], got %s" % (Ls, hist_i.shape))
        self.Sn = int(hist_i_new.shape[1])
        self.u = t(u, torch.int32)
        self.i = t(i, torch.int32)
        self.hist_i = t(hist_i, torch.int32)
        self.hist_i_new = t(hist_i_new, torch.int32) if self.Sn > 0 else torch.zeros(1, dtype=torch.int32, device=device)
        self.hist_t = t(hist_t, torch.float32)
        self.sl = t(sl, torch.int32)
        self.sl_new = t(new_sl, torch.int32)
        self.u_cate = t(c, torch.int32)
        self.j = t(yj, torch.int32) if is_test else None
        self.y = None if is_test else t(yj, torch.float32)
        self.c = self.struct()

    @classmethod
    def allocate(cls, B, Sn, Ls, device, is_test=False):
        """Uninitialised device arrays of a [B, Ls] / [B, Sn] batch (filled by tlsan_batch_pack)."""
        self = cls.__new__(cls)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)
        self.B, self.Sn = int(B), int(Sn)
        self.u, self.i = e(B, torch.int32), e(B, torch.int32)
        self.hist_i = e((B, Ls), torch.int32)
        self.hist_i_new = e((B, Sn), torch.int32) if Sn > 0 else torch.zeros(1, dtype=torch.int32, device=device)
        self.hist_t = e((B, Ls), torch.float32)
        self.sl, self.sl_new, self.u_cate = e(B, torch.int32), e(B, torch.int32), e(B, torch.int32)
        self.j = e(B, torch.int32) if is_test else None
        self.y = None if is_test else e(B, torch.float32)
        self.c = self.struct()
        return self

    def to_host(self):
        """The reference's 9-tuple (input.py:54 / :107) as numpy arrays."""
        n = lambda t: t.cpu().numpy()
        third = n(self.j).astype(np.int64) if self.j is not None else n(self.y).astype(np.int64)
        hin = n(self.hist_i_new).astype(np.int64).reshape(self.B, self.Sn) if self.Sn > 0 else np.zeros((self.B, 0), np.int64)
        return (n(self.u).astype(np.int64), n(self.i).astype(np.int64), third, n(self.hist_i).astype(np.int64), hin,
                n(self.hist_t), n(self.sl).astype(np.int64), n(self.sl_new).astype(np.int64), n(self.u_cate).astype(np.int64))

    def __len__(self):
        return self.B

    def struct(self, use_j=True):
        p = lambda x: None if x is None else x.data_ptr()
        return L.Batch(self.B, self.Sn, p(self.u), p(self.i), p(self.j) if use_j else None, p(self.y),
                       p(self.hist_i), p(self.hist_i_new), p(self.hist_t), p(self.sl), p(self.sl_new),
                       p(self.u_cate))


def _flushing(name):
    """A Model tensor (tables, dense parameters, state) as an attribute whose READ first makes the correction a clipped
    two-launch step may owe (Model._flush): whoever takes the tensor sees the reference's update.  The training step
    itself goes by the raw tensors and pointers."""
    raw = "_" + name

    def get(self):
        if raw not in self.__dict__:
            raise AttributeError(name)      # (hasattr before the tensor exists, as any attribute answers)
        self._flush()
        return self.__dict__[raw]

    def put(self, value):
        self.__dict__[raw] = value
    return property(get, put)


class Model(object):
    _fix_owed = False     # a training step ran since the last flush (_flush)
    item_emb, item_b, user_emb, usert_emb, cate_emb = (_flushing(k) for k in ("item_emb", "item_b", "user_emb", "usert_emb", "cate_emb"))
    dense, state = _flushing("dense"), _flushing("state")

    def __init__(self, config, item_cate_list, device="cuda:0", seed=1234, norm_mode="tf18", l2_mode="dense",
                 table_dtype="f32", init="numpy", matrix_dtype="f32"):
        """table_dtype: "f32" (the reference's precision) or "bf16" -- item_emb / user_emb / cate_emb stored
        as bfloat16 (BASELINE.json configs[2]), arithmetic in fp32, updates written back with
        deterministic stochastic rounding; usert_emb, item_b and the dense weights stay fp32.
        init: "numpy" -- the variables' initial values drawn on the host (init_params; reproducible across
        devices); "device" -- the same distributions drawn in HBM (tables of 10^7 rows: BASELINE.json
        configs[4]; no host copy of the tables is ever made).
        config["optimizer"]: "sgd", "adam", "rmsprop", "adadelta" (the reference's), or "lazy_adam", "lazy_rmsprop",
        "lazy_adadelta": the same optimizers restricted to the rows each batch used (unused rows keep their values and
        slots bit for bit; include/tlsan.h, TLSAN_OPT_LAZY), or "lazy_adagrad", "lazy_rowwise_adagrad": Adagrad on the used
        rows with one accumulator per element / per table row.  A lazy optimizer runs the lazy tail whatever l2_mode
        says: "dense" and "lazy" are both accepted, with the same result; norm_mode must be "tf18"."""
        if init not in ("numpy", "device"):
            raise ValueError("init must be 'numpy' or 'device'")
        # matrix_dtype: arithmetic of the fused kernel's matrix products -- "f32": exact fp32 MFMA (the reference's
        # precision); "bf16": operands rounded to bfloat16, fp32 products and sums (include/tlsan.h,
        # tlsan_params.matrix_dtype).  An extension for BASELINE.json configs[2]; any window the kernels take (in registers or streamed), with or without dropout.
        if matrix_dtype not in ("f32", "bf16"):
            raise ValueError("matrix_dtype must be 'f32' or 'bf16'")
        self.matrix_dtype = matrix_dtype
        if table_dtype not in ("f32", "bf16"):
            raise ValueError("table_dtype must be 'f32' or 'bf16'")
        self.table_dtype = table_dtype
        self.config = config
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise RuntimeError("tlsan_amd.Model needs a GPU (no CPU fallback)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        if config.get("num_blocks", 1) != 1:
            raise ValueError("num_blocks != 1 is degenerate in the reference (model.py:330-364) and unsupported")
        self.dropout = float(config.get("dropout", 0.0))           # model.py:116-118, 428-431
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self._seed = int(seed)
        self.optimizer = config.get("optimizer", "sgd")           # model.py:188-195
        if self.optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of %s" % (sorted(OPTIMIZERS),))
        # lazy_adam / lazy_rmsprop / lazy_adadelta update only the rows a batch used (include/tlsan.h, TLSAN_OPT_LAZY): they
        # always run the lazy tail, whatever l2_mode says -- "dense" and "lazy" are both accepted and give the same result
        self.lazy_opt = self.optimizer in LAZY_OPTIMIZERS or self.optimizer in LAZY_ADAGRAD_OPTIMIZERS
        if self.lazy_opt:
            if l2_mode not in ("dense", "lazy"):
                raise ValueError("l2_mode must be 'dense' or 'lazy'")
            if norm_mode != "tf18":
                raise NotImplementedError("optimizer=%r supports norm_mode='tf18' only" % self.optimizer)
            l2_mode = "lazy"
        elif self.optimizer != "sgd":
            # adam / rmsprop / adadelta see every row of the regularised tables every step (the L2 term
            # makes the reference's gradients dense), so the lazy-L2 form does not apply
            if l2_mode != "dense":
                raise NotImplementedError("optimizer=%r needs l2_mode='dense'" % self.optimizer)
        self.train_writer = _Writer(os.path.join(config.get("model_dir", "."), "train"))
        self.eval_writer = _Writer(os.path.join(config.get("model_dir", "."), "eval"))
        d = config["hidden_units"]
        self.dims = L.Dims(config["user_count"], config["item_count"], config["cate_count"], d,
                           config["itemid_embedding_size"], config["cateid_embedding_size"],
                           config["num_heads"], config["Ls"])
        if config["userid_embedding_size"] != config["itemid_embedding_size"]:
            raise ValueError("userid_embedding_size must equal itemid_embedding_size (both + cate = hidden_units)")
        self.lay = L.DenseLayout()
        L.check(self.lib.tlsan_dense_layout_of(C.byref(self.dims), C.byref(self.lay)), "tlsan_dense_layout_of")
        nbytes = self.lib.tlsan_state_bytes(C.byref(self.dims))
        if nbytes == 0:
            raise L.TlsanError("unsupported configuration: %s" % self.lib.tlsan_last_error().decode())
        self.norm_mode = {"tf18": L.NORM_TF18, "dedup": L.NORM_DEDUP}[norm_mode]
        # l2_mode: "dense" decays every row every step like the reference's dense L2 gradient
        # (model.py:164-172); "lazy" is the same update kept as W = P * W_stored (one global scale),
        # touching only rows that received a gradient -- identical up to fp32 rounding.
        self.l2_mode = {"dense": L.L2_DENSE, "lazy": L.L2_LAZY}[l2_mode]
        if self.l2_mode == L.L2_LAZY and self.norm_mode != L.NORM_TF18:
            raise NotImplementedError("l2_mode='lazy' supports norm_mode='tf18' only")
        icl = np.asarray(item_cate_list, np.int32)
        if icl.shape != (config["item_count"],):
            raise ValueError("item_cate_list must be [item_count]")
        self.item_cate = torch.as_tensor(icl).to(self.device)
        self._alloc_params()
        if init == "numpy":
            self.set_params(self.init_params(config, seed))
        else:
            self._init_on_device(config, seed)
        self._alloc_slots()
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        if self.l2_mode == L.L2_LAZY:
            self.cparams.scale = self.lib.tlsan_state_scale(self.state.data_ptr())
        self._ws = None
        self._ws_key = (0, 0)
        self.renorm_every = 4096   # lazy L2: fold the table scale into the tables every so many steps (0 = never)
        # two destination-index slots: the current step's and the one being built for the next batch
        self._idx_slot = 0
        self._idx_ready = [None] * L.INDEX_SLOTS     # batch whose destination index sits (or is being built) in the slot
        self._idx_event = [torch.cuda.Event() for _ in range(L.INDEX_SLOTS)]
        self._pre_event = torch.cuda.Event()
        # host-visible word the first kernel of a step writes its sequence number into (train_async)
        self._started = torch.zeros(16, dtype=torch.int32).pin_memory()
        # (a step still queued when the Model is dropped writes this word when it starts: the pinned block must not be
        #  recycled under it -- the word outlives the Model, 64 bytes per Model ever built)
        _STARTED_WORDS.append(self._started)
        self._started_addr = self._started.data_ptr()
        self._started_word = C.c_uint32.from_address(self._started_addr)
        self._start_seq = 0
        self.poll_seconds = 0.0     # time train_async spent polling the `started` word (the host waiting for the GPU)
        self.started_at = None      # a list: train_async appends the host time at which it saw each step's first kernel start
        self._side = None
        self._step = 0
        self._epoch = 0
        self.global_step = _Var(lambda: self._step)
        self.global_epoch_step = _Var(lambda: self._epoch)
        self.global_epoch_step_op = _Var(self._inc_epoch)
        self._out = torch.zeros(4, dtype=torch.float32, device=self.device)  # loss, gnorm, sq_rows
        self._topk = c = TopKCounters()
        for idx, k in enumerate(KS):            # (0 before any batch was counted)
            setattr(self, "prec_%d" % k, _Var(lambda idx=idx, k=k: c.hits_p[idx] / max(1, k * c.n_p)))
            setattr(self, "recall_%d" % k, _Var(lambda idx=idx: c.hits_r[idx] / max(1, c.n_r)))
        self._sync_state()

    # ------------------------------------------------------------------ parameters
    @staticmethod
    def init_params(config, seed=1234):
        """Variables of model.py:58-81, :443-450, :347 with the reference's initial values."""
        rng = np.random.RandomState(seed)
        I, U, Cc = config["item_count"], config["user_count"], config["cate_count"]
        di, dc = config["itemid_embedding_size"], config["cateid_embedding_size"]
        d, H, Ls = config["hidden_units"], config["num_heads"], config["Ls"]
        dh = d // H
        p = {
            "gamma": np.ones((), np.float32),
            "item_emb": glorot_uniform(rng, (I, di)),
            "item_b": np.zeros(I, np.float32),
            "user_emb": glorot_uniform(rng, (U, di)),
            "usert_emb": -np.ones((U, Ls), np.float32),
            "cate_emb": glorot_uniform(rng, (Cc, dc)),
            "dense_K": glorot_uniform(rng, (d, d)),
            "dense_b": np.zeros(d, np.float32),
        }
        for blk in ("fwa1", "fwa2"):
            p[blk + "_W1"] = glorot_uniform(rng, (dh, dh))
            p[blk + "_b1"] = np.zeros(dh, np.float32)
            p[blk + "_W2"] = glorot_uniform(rng, (dh, dh))
            p[blk + "_b2"] = np.zeros(dh, np.float32)
        return p

    def _init_on_device(self, config, seed):
        """init_params' distributions (glorot-uniform tables, usert_emb = -1, item_b = 0) drawn on the device;
        the small dense weights still come from the host stream."""
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed))
        for t in (self.item_emb, self.user_emb, self.cate_emb):
            limit = float(np.sqrt(6.0 / (t.shape[0] + t.shape[1])))
            if t.dtype == torch.float32:
                t.uniform_(-limit, limit, generator=g)
            else:
                t.copy_(torch.empty(t.shape, dtype=torch.float32, device=self.device).uniform_(-limit, limit, generator=g))
        self.item_b.zero_()
        self.usert_emb.fill_(-1.0)
        small = dict(config, item_count=1, user_count=1, cate_count=1)
        self.dense.copy_(torch.as_tensor(self.pack_dense(self.init_params(small, seed))))

    def _alloc_params(self):
        cfg, dev = self.config, self.device
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        tdt = torch.bfloat16 if self.table_dtype == "bf16" else torch.float32
        zt = lambda *s: torch.zeros(*s, dtype=tdt, device=dev)
        self.item_emb = zt(cfg["item_count"], cfg["itemid_embedding_size"])
        self.item_b = z(cfg["item_count"])
        self.user_emb = zt(cfg["user_count"], cfg["itemid_embedding_size"])
        self.usert_emb = z(cfg["user_count"], cfg["Ls"])
        self.cate_emb = zt(cfg["cate_count"], cfg["cateid_embedding_size"])
        self.dense = z(self.lay.n_dense)
        self.dense_KT = z(cfg["hidden_units"], cfg["hidden_units"])
        self.cparams = L.Params(self.item_emb.data_ptr(), self.item_b.data_ptr(), self.user_emb.data_ptr(),
                                self.usert_emb.data_ptr(), self.cate_emb.data_ptr(), self.dense.data_ptr(),
                                self.dense_KT.data_ptr(), self.item_cate.data_ptr(), 0, 0, 0, 0, None,
                                L.TABLE_BF16 if self.table_dtype == "bf16" else L.TABLE_F32,
                                L.MATRIX_BF16 if self.matrix_dtype == "bf16" else L.MATRIX_F32)

    def _alloc_slots(self):
        """Accumulators of adam / rmsprop / adadelta (tlsan_optimizer in include/tlsan.h): two sets of
        tables shaped like the parameters; RMSProp's first slot starts at one as in TF 1.8.  The Adagrad forms keep ONE
        set, filled with TF's initial_accumulator_value; lazy_rowwise_adagrad's four tables are [rows] vectors."""
        self.slots = None
        self._copt = None
        if self.optimizer == "sgd":
            return
        self.slots, self._cslots = [], []
        adagrad = self.optimizer in LAZY_ADAGRAD_OPTIMIZERS
        row_slots = self.optimizer == "lazy_rowwise_adagrad"
        for which in range(1 if adagrad else 2):
            fill = 1.0 if (self.optimizer in ("rmsprop", "lazy_rmsprop") and which == 0) else 0.0
            if adagrad:
                fill = ADAGRAD_INITIAL_ACCUMULATOR
            t = {k: torch.full_like(getattr(self, k), fill, dtype=torch.float32) for k in TABLE_KEYS}
            if row_slots:
                for k in ROW_SLOT_KEYS:
                    t[k] = torch.full((getattr(self, k).shape[0],), fill, dtype=torch.float32, device=self.device)
            t["dense"] = torch.full_like(self.dense, fill)
            self.slots.append(t)
            self._cslots.append(L.Params(t["item_emb"].data_ptr(), t["item_b"].data_ptr(), t["user_emb"].data_ptr(),
                                         t["usert_emb"].data_ptr(), t["cate_emb"].data_ptr(), t["dense"].data_ptr(),
                                         None, None, 0, 0, 0, 0, None, L.TABLE_F32))
        kind, b1, b2, eps = OPTIMIZERS[self.optimizer]
        self._copt = L.Optimizer(kind, 0, b1, b2, eps, C.addressof(self._cslots[0]),
                                 None if adagrad else C.addressof(self._cslots[1]))

    def _flush(self):
        """A clipped lazy-L2 SGD step in the two-launch form leaves its correction to the next step's fused kernel
        (include/tlsan.h, tlsan_train_step): make it now -- one short launch on the current stream, nothing when no step
        ran since the last flush.  Everything that reads the tables, the dense parameters or the state other than the
        next training step comes through here: the accessors below, the forward, grads, the checkpoint, a graph capture."""
        if self._fix_owed:
            self._fix_owed = False
            L.check(self.lib.tlsan_state_flush(C.byref(self.dims), C.byref(self.cparams), self._state.data_ptr(),
                                               self._stream()), "tlsan_state_flush")

    def _train_call(self, db, hp, out, ws):
        # (only the lazy-L2 SGD step has the two-launch form; a library without the call -- an older build loaded for an
        #  A/B -- has no such form either)
        self._fix_owed = self.l2_mode == L.L2_LAZY and self._copt is None and hasattr(self.lib, "tlsan_state_flush")
        if self._copt is None:
            L.check(self.lib.tlsan_train_step(C.byref(self.dims), C.byref(self.cparams), C.byref(db.c), C.byref(hp),
                                              C.byref(out), self._state.data_ptr(), ws.data_ptr(), ws.numel(),
                                              self._stream()), "tlsan_train_step")
        else:
            self._copt.step = self._step + 1      # Adam's beta powers: updates applied so far + 1
            L.check(self.lib.tlsan_train_step_opt(C.byref(self.dims), C.byref(self.cparams), C.byref(db.c), C.byref(hp),
                                                  C.byref(self._copt), C.byref(out), self._state.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), self._stream()), "tlsan_train_step_opt")

    def get_slots(self):
        """The optimizer's accumulators as a list of dicts of numpy arrays named like the parameters: two, the Adagrad
        forms one (lazy_rowwise_adagrad: the four tables' entries are [rows] arrays); None for sgd."""
        if self.slots is None:
            return None
        out = []
        for t in self.slots:
            d = {k: t[k].cpu().numpy().copy() for k in TABLE_KEYS}
            d.update(self.unpack_dense(t["dense"].cpu().numpy()))
            out.append(d)
        return out

    def _check_slots(self, slots):
        """Slot sets as get_slots returns them (a checkpoint's) must be this optimizer's: as many, shaped alike."""
        if len(slots) != len(self.slots):
            raise ValueError("%d slot set(s) do not fit optimizer=%r, which keeps %d" % (len(slots), self.optimizer, len(self.slots)))
        for n, (t, src) in enumerate(zip(self.slots, slots), 1):
            for k in TABLE_KEYS:
                if tuple(np.shape(src[k])) != tuple(t[k].shape):
                    raise ValueError("slot%d/%s of shape %s does not fit optimizer=%r, whose accumulator has shape %s"
                                     % (n, k, tuple(np.shape(src[k])), self.optimizer, tuple(t[k].shape)))

    def set_slots(self, slots):
        self._check_slots(slots)      # (before anything is copied)
        for t, src in zip(self.slots, slots):
            for k in TABLE_KEYS:
                t[k].copy_(torch.as_tensor(np.asarray(src[k], np.float32)))
            t["dense"].copy_(torch.as_tensor(self.pack_dense(src)))

    def pack_dense(self, p):
        return pack_dense(self.lay, self.config["hidden_units"], self.config["num_heads"], p)

    def unpack_dense(self, flat):
        return unpack_dense(self.lay, self.config["hidden_units"], self.config["num_heads"], flat)

    def set_params(self, p):
        """Load a dict of numpy arrays (names as in oracle / checkpoint) into device memory."""
        for k in TABLE_KEYS:
            t = getattr(self, k)
            a = np.asarray(p[k], np.float32)
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError("%s: shape %s != %s" % (k, a.shape, tuple(t.shape)))
            t.copy_(torch.as_tensor(a))      # (bf16 tables: round to nearest even on load)
        self.dense.copy_(torch.as_tensor(self.pack_dense(p)))
        if hasattr(self, "state"):
            self._sync_state()

    def fold_scale(self):
        """lazy L2: fold the table scale P into the stored tables (P = 1 afterwards).  The lazy optimizers keep P = 1:
        nothing to fold."""
        self._flush()
        if self.l2_mode == L.L2_LAZY and not self.lazy_opt:
            L.check(self.lib.tlsan_state_renorm(C.byref(self.dims), C.byref(self.cparams), self.state.data_ptr(),
                                                self._stream()), "tlsan_state_renorm")

    def table_scale(self):
        return float(self.state[:4].view(torch.float32).item())

    def get_params(self):
        self.fold_scale()
        out = {k: getattr(self, k).detach().float().cpu().numpy().copy() for k in TABLE_KEYS}
        out.update(self.unpack_dense(self.dense.detach().cpu().numpy()))
        return out

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _sync_state(self):
        self._fix_owed = False     # (the state is cleared: whatever a step owed goes with it)
        # tlsan_state_init clears the whole state, both destination-index slots included: an index that was
        # prefetched for an announced successor (train_async(next_batch=)) is gone with it -- wait for the side
        # stream to be done with the slot, then forget the announcement (the next step builds its index inline)
        for k in range(L.INDEX_SLOTS):
            if self._idx_ready[k] is not None:
                self._idx_event[k].synchronize()
        self._idx_ready = [None] * L.INDEX_SLOTS
        L.check(self.lib.tlsan_state_init(C.byref(self.dims), C.byref(self.cparams), self.state.data_ptr(),
                                          self._stream()), "tlsan_state_init")

    def _workspace(self, B, Sn):
        kB, kS = self._ws_key
        if self._ws is None or B > kB or Sn > kS:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the workspace cannot grow during capture (capture_step sizes it first)")
            kB, kS = max(B, kB), max(Sn, kS)
            n = self.lib.tlsan_workspace_bytes(C.byref(self.dims), kB, kS)
            if n == 0:
                raise L.TlsanError("tlsan_workspace_bytes: %s" % self.lib.tlsan_last_error().decode())
            self._flush()     # (an owed correction reads the last step's gradient rows in the old block)
            torch.cuda.synchronize(self.device)
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._ws_key = (kB, kS)
        return self._ws

    def _inc_epoch(self):
        self._epoch += 1
        return self._epoch

    def dropout_seed(self, step=None):
        """Seed of the keep / drop pattern of update number `step` (default: the next one): a fixed
        function of the model's seed and the step, so that runs are reproducible."""
        step = self._step if step is None else step
        return ((self._seed * 0x9E3779B1) ^ ((step + 1) * 0x85EBCA77)) & 0xFFFFFFFF

    def hparams(self, lr, index_slot=0, index_prebuilt=0):
        return L.HParams(float(lr), float(self.config["regulation_rate"]), float(self.config["max_gradient_norm"]),
                         self.norm_mode, self.l2_mode, index_slot, index_prebuilt,
                         self.dropout, self.dropout_seed() if self.dropout > 0.0 else 0)

    # ------------------------------------------------------------------ training
    def device_batch(self, batch, is_test=False):
        return batch if isinstance(batch, DeviceBatch) else DeviceBatch(batch, self.device, is_test, self.config["Ls"])

    def train_async(self, batch, lr, logits=None, next_batch=None, after_next=None):
        """Enqueue one step (model.py:208-234) without reading the loss back.

        next_batch (optional, what an input pipeline knows anyway): its destination index (use
        counts, segment offsets -- a function of the ids only) is built on a second stream while
        this step computes, so the next step starts directly with the fused kernel.  The two
        streams are ordered by HOST waits on events that are complete by the time they are
        needed (device-side event waits between queues cost more than the work they would hide).

        after_next (optional): the batch after next_batch.  Its index is built TWO steps ahead.  With one batch ahead
        the index of batch t+1 can only run once k_fwd_bwd of step t has left the GPU (that kernel fills every CU), and
        step t+1 is launched when the host has seen it finish: kernel -> index (12 us) -> host wake-up -> launch is a
        path as long as the step's own kernels, so shortening either alone changes nothing.  Two ahead, the index a
        step waits for was finished during the previous step and the main stream never idles."""
        db = self.device_batch(batch)
        ws = self._workspace(db.B, db.Sn)
        out = L.StepOut(self._out.data_ptr(), self._out.data_ptr() + 4, None if logits is None else logits.data_ptr(), None)
        if torch.cuda.is_current_stream_capturing():   # hipGraph capture: one self-contained step
            if self.dropout > 0.0:
                raise NotImplementedError("the dropout seed is a launch argument: capture is not supported")
            if self.optimizer in ("adam", "lazy_adam"):
                raise NotImplementedError("Adam's step count is a launch argument: capture is not supported")
            hp = self.hparams(lr)
            self._train_call(db, hp, out, ws)
            self._step += 1
            return db
        if self.l2_mode == L.L2_LAZY and not self.lazy_opt and self.renorm_every and self._step and \
                self._step % self.renorm_every == 0:
            # keep the table scale P = prod(1 - lr c reg) away from fp32 underflow in very long runs
            # (a fixed schedule, so runs stay bitwise reproducible); one sweep of the tables
            self.fold_scale()
        k = self._idx_slot
        if self._idx_ready[k] is not None and self._idx_ready[k] is not db:
            raise RuntimeError("train_async: the batch announced as next_batch must be the next one trained "
                               "(its destination index is already counted into the state)")
        pre = self._idx_ready[k] is db
        # streams are ordered by HOST waits on events that are complete by the time they are needed (a device-side
        # cross-queue wait costs ~8 us on this stack: measured, worse); under stream capture the host cannot wait
        dev_wait = torch.cuda.is_current_stream_capturing()
        if pre:
            if dev_wait:
                torch.cuda.current_stream(self.device).wait_event(self._idx_event[k])
            else:
                self._idx_event[k].synchronize()       # the side stream finished this batch's index
        self._idx_ready[k] = None
        main = torch.cuda.current_stream(self.device)
        NS = L.INDEX_SLOTS
        ahead = []      # (batch, slot) whose index is not there yet
        for j, nb in enumerate((next_batch, after_next)):
            if nb is None:
                continue
            kk = (k + 1 + j) % NS
            ndb = self.device_batch(nb)
            if self._idx_ready[kk] is ndb:
                continue
            if self._idx_ready[kk] is not None:
                raise RuntimeError("train_async: the batches announced ahead must be trained in that order "
                                   "(the destination index of another batch is already counted into the state)")
            ahead.append((ndb, kk))
        # everything queued so far -- the previous steps (last users of the free index slots) and whatever produced the
        # announced batches' arrays -- must be done before the side stream reads them.  An event recorded here would be
        # a barrier packet between the previous step's last kernel and this step's first one (measured: the fused
        # kernel starts 6.6 us after its predecessor ends instead of < 2); instead the step's first kernel stores a
        # sequence number into a pinned host word when it begins to run (tlsan_step_out.started), and the host polls it.
        # (under stream capture nothing runs, so the word would never change: events are the capturable path)
        flag_wait = bool(ahead) and not dev_wait
        if ahead and not flag_wait:
            self._pre_event.record(main)
        if flag_wait:
            self._start_seq = (self._start_seq + 1) & 0x7FFFFFFF
            out.started = self._started_addr
            out.started_value = self._start_seq
        hp = self.hparams(lr, k, 1 if pre else 0)
        self._train_call(db, hp, out, ws)
        if ahead:
            if self._side is None:
                # (high priority: the index kernels are short and the NEXT step cannot start without them; left at
                #  the default they trail behind the 2400 workgroups of the row-sum / update launches they share
                #  the GPU with -- measured: no difference either way)
                self._side = concurrent_streams(self.device, 1, priority=-1)[0]
            if dev_wait:
                self._side.wait_event(self._pre_event)
            else:
                word, want, t0, polls = self._started_word, self._start_seq, None, 0
                tp = time.perf_counter()
                while word.value != want:
                    polls += 1
                    if polls & 255:
                        continue
                    time.sleep(0)            # (every 256 polls: let another Python thread have the GIL)
                    if t0 is None:
                        t0 = time.perf_counter()
                    elif time.perf_counter() - t0 > 30.0:
                        raise RuntimeError("train_async: the step's first kernel did not start within 30 s")
                tq = time.perf_counter()
                self.poll_seconds += tq - tp     # (waiting for the GPU, not host work: bench.py subtracts it)
                if self.started_at is not None:  # (when the host SAW this step's first kernel start: bench.py's spread of step times)
                    self.started_at.append(tq)
            for ndb, kk in ahead:
                flag = L.INDEX_FOR_LAZY_SGD if (self.l2_mode == L.L2_LAZY and (self.optimizer == "sgd" or self.lazy_opt)) else 0
                L.check(self.lib.tlsan_batch_index(C.byref(self.dims), C.byref(ndb.c), self.cparams.item_cate, self._state.data_ptr(), kk | flag,
                                                   C.c_void_p(self._side.cuda_stream)), "tlsan_batch_index")
                self._idx_event[kk].record(self._side)
                self._idx_ready[kk] = ndb
        self._idx_slot = (k + 1) % L.INDEX_SLOTS
        self._step += 1
        return db

    def capture_step(self, batch, lr):
        """Capture one training step on `batch` into a hipGraph (fork/join of the index-build
        side stream included) and return the graph: `g.replay()` re-runs the step on the same
        device buffers.  lr is baked in (re-capture when it changes, train.py:232-233).
        A lazy-L2 SGD step in the two-launch form may leave a correction owed (_flush).  The captured step builds its own
        index, so the library records its flush launch in the graph in front of the step, whatever the state owed on the
        day of the capture (include/tlsan.h, tlsan_state_flush): replay after replay is right by what the graph holds, and
        replay() marks the model as owing for everything else that reads."""
        db = self.device_batch(batch)
        self._flush()
        # the graph bakes the workspace pointer in: size it for the worst case of this batch size once (the
        # longest session the kernels take, TLSAN_SN_CAP), so that a later, longer batch cannot make
        # _workspace() reallocate it under graphs captured earlier
        self._workspace(db.B, max(db.Sn, L.SN_CAP))
        self.train_async(db, lr)          # warm: lazy one-time initialisation happens outside capture
        self._step -= 1
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.train_async(db, lr)
        self._step -= 1
        g._tlsan_batch = db               # keep the captured buffers alive
        g._tlsan_ws = self._ws            # ... and the workspace the graph writes to
        return g

    def replay(self, g):
        if g._tlsan_ws is not self._ws:
            # a larger batch made the workspace grow after the capture: the graph's block stays alive (pinned
            # above), but it is no longer the model's -- recapture rather than run on a stale pointer
            raise RuntimeError("replay: the workspace was reallocated after this graph was captured; recapture the step")
        g.replay()
        self._fix_owed = self.l2_mode == L.L2_LAZY and self._copt is None and hasattr(self.lib, "tlsan_state_flush")
        self._step += 1

    def train(self, sess, batch, lr, add_summary=False):
        self.train_async(batch, lr)
        loss = float(self._out[0].item())
        if add_summary:
            self.train_writer.add_summary(self.train_summary(loss), global_step=self._step)
        return loss

    def train_summary(self, loss=None):
        """model.py:174-183's merged summary as (tag, value) pairs: the two scalars, and for every
        histogram its count / min / max / mean / std (`attention_output`, the histogram of u_t, needs
        a forward pass of the batch and is not kept)."""
        P = float(self.state[:4].view(torch.float32).item()) if self.l2_mode == L.L2_LAZY else 1.0
        out = []
        l2 = 0.0
        for tag, t in (("embedding/1_item_emb", self.item_emb), ("embedding/2_user_emb", self.user_emb),
                       ("embedding/3_cate_emb", self.cate_emb), ("embedding/4_usert_emb", self.usert_emb)):
            v = t.float() * P                              # true parameter = P * stored (lazy L2)
            l2 += 0.5 * float(v.double().pow(2).sum().item())     # tf.nn.l2_loss (model.py:164-169)
            for name, x in (("count", v.numel()), ("min", v.min().item()), ("max", v.max().item()),
                            ("mean", v.mean().item()), ("std", v.std().item())):
                out.append(("%s/%s" % (tag, name), float(x)))
        out.append(("gamma", float(self.dense[self.lay.gamma].item())))
        out.append(("L2_norm_user_item", l2))
        out.append(("Training Loss", float(self._out[0].item()) if loss is None else float(loss)))
        return out

    def last_gnorm(self):
        return float(self._out[1].item())

    def grads(self, batch, lr=1.0):
        """tf.gradients(loss, trainables) (model.py:198) as numpy arrays; test/diagnostic API."""
        db = self.device_batch(batch)
        self._flush()
        ws = self._workspace(db.B, db.Sn)
        g = {k: torch.zeros_like(getattr(self, k), dtype=torch.float32) for k in TABLE_KEYS}
        gd = torch.zeros_like(self.dense)
        logits = torch.zeros(db.B, dtype=torch.float32, device=self.device)
        go = L.GradsOut(g["item_emb"].data_ptr(), g["item_b"].data_ptr(), g["user_emb"].data_ptr(),
                        g["usert_emb"].data_ptr(), g["cate_emb"].data_ptr(), gd.data_ptr())
        out = L.StepOut(self._out.data_ptr(), self._out.data_ptr() + 4, logits.data_ptr(), self._out.data_ptr() + 8)
        # (an index slot at rest: the other one may hold the index prefetched for an announced next batch)
        free = [k for k in range(L.INDEX_SLOTS) if self._idx_ready[k] is None]
        if not free:
            raise RuntimeError("grads: every index slot holds a prefetched index")
        slot = free[0]
        hp = self.hparams(lr, slot, 0)
        L.check(self.lib.tlsan_grads(C.byref(self.dims), C.byref(self.cparams), C.byref(db.c), C.byref(hp),
                                     C.byref(go), C.byref(out), self.state.data_ptr(), ws.data_ptr(), ws.numel(),
                                     self._stream()), "tlsan_grads")
        res = {k: v.cpu().numpy() for k, v in g.items()}
        res.update(self.unpack_dense(gd.cpu().numpy()))
        o = self._out.cpu().numpy()
        return dict(grads=res, loss=float(o[0]), gnorm=float(o[1]), logits=logits.cpu().numpy())

    # ------------------------------------------------------------------ evaluation
    def forward(self, batch, is_test=True, want_u_t=False, want_att=False):
        """logits for candidate i (and j when the batch has one) -- `sess.run(self.logits)`.
        want_att: also leave the reference's two attention-weight tensors (model.py:122, 386-394) on the model:
        self.att0 [H*B, Ls, d/H] and self.att1 [H*B, 1+Sn, d/H], row h*B + b (`sess.run([model.att0, model.att1])`)."""
        db = self.device_batch(batch, is_test)
        self._flush()
        li = torch.empty(db.B, dtype=torch.float32, device=self.device)
        lj = torch.empty(db.B, dtype=torch.float32, device=self.device) if db.j is not None else None
        ut = torch.empty(db.B, self.config["hidden_units"], dtype=torch.float32, device=self.device) if want_u_t else None
        a0 = a1 = None
        if want_att:
            H, dh = self.config["num_heads"], self.config["hidden_units"] // self.config["num_heads"]
            a0 = torch.empty(H * db.B, self.config["Ls"], dh, dtype=torch.float32, device=self.device)
            a1 = torch.empty(H * db.B, 1 + db.Sn, dh, dtype=torch.float32, device=self.device)
        L.check(self.lib.tlsan_forward_att(C.byref(self.dims), C.byref(self.cparams), C.byref(db.c), li.data_ptr(),
                                           None if lj is None else lj.data_ptr(), None if ut is None else ut.data_ptr(),
                                           None if a0 is None else a0.data_ptr(), None if a1 is None else a1.data_ptr(),
                                           None, 0, self._stream()), "tlsan_forward")
        if want_att:
            self.att0, self.att1 = a0, a1
        return li, lj, ut, db

    def eval_auc(self, sess, batch):
        """mean(logit(pos) - logit(neg) > 0), ties wrong (model.py:237-263)."""
        return float(self.pairs_ranked_right(batch).float().mean().item())

    def pairs_ranked_right(self, batch):
        """Per test row: logit(pos) - logit(neg) > 0 (bool tensor on the device) -- what eval_auc averages.  A row's
        value does not depend on which other rows share its batch, so the driver evaluates in large launches and forms
        the reference's per-batch means from slices (train.eval_auc)."""
        li, lj, _, _ = self.forward(batch, is_test=True)
        return (li - lj) > 0

    def label_ranks(self, batch, exclude=None, return_eligible=False):
        """rank of the positive item among all items for each test row (model.py:140-156) -> [B] int32 device tensor.
        exclude=None: among ALL items (the reference's ranking).  Otherwise exclude takes recommend's forms ("history",
        a sequence of B id arrays, a SeenItems holder) and the result is the FILTERED rank: the label's rank among the
        items that are not excluded -- the all-items rank minus the listed items the rank kernel counted ahead of the
        label (tlsan_eval_ranks_excl), so it is exact, never negative, and 0 when everything but the label is listed.
        The label itself is never excluded, even when the list holds it (test labels often sit in their user's own
        seen list).  return_eligible: also the number of items each row's label competes with,
        item_count - 1 - |list \\ {label}| -> (ranks, eligible)."""
        li, lj, ut, db = self.forward(batch, is_test=True, want_u_t=True)
        ws = self._workspace(db.B, db.Sn)
        ranks = torch.empty(db.B, dtype=torch.int32, device=self.device)
        if exclude is None:
            L.check(self.lib.tlsan_eval_ranks(C.byref(self.dims), C.byref(self.cparams), ut.data_ptr(), db.i.data_ptr(),
                                              db.B, ranks.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                    "tlsan_eval_ranks")
            if return_eligible:
                return ranks, torch.full_like(ranks, self.config["item_count"] - 1)
            return ranks
        off, xid = exclusion_csr(db, exclude, self.config["item_count"])
        ahead, held = torch.empty_like(ranks), torch.empty_like(ranks)
        L.check(self.lib.tlsan_eval_ranks_excl(C.byref(self.dims), C.byref(self.cparams), ut.data_ptr(), db.i.data_ptr(),
                                               db.B, off.data_ptr(), xid.data_ptr(), ranks.data_ptr(), ahead.data_ptr(),
                                               held.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                "tlsan_eval_ranks_excl")
        ranks = ranks - ahead
        return (ranks, (self.config["item_count"] - 1) - held) if return_eligible else ranks

    def item_scope(self, items=None, mask=None, categories=None):
        """An ItemScope over this model's items: from ids, a bool mask, or category ids (with the model's item_cate)."""
        return ItemScope(self.config["item_count"], self.device, items=items, mask=mask, categories=categories,
                         item_cate=None if categories is None else self.item_cate)

    def item_boost(self, values=None, items=None, categories=None, base=0.0):
        """An ItemBoost over this model's items, on its device: from values ([item_count] numbers), from items=(ids,
        values) against `base` (ItemBoost.of_items), or from categories=[cate_count] values through the model's item_cate
        (ItemBoost.of_categories).  Exactly one of the three."""
        return item_boost_for(self.config["item_count"], self.device, lambda: self.item_cate, values, items, categories, base)

    def last_item_categories(self, batch):
        """last_item_categories of a batch (tuple or DeviceBatch) with this model's item -> category map."""
        return last_item_categories(self.device_batch(batch, is_test=True), self.item_cate)

    def category_index(self, within=None):
        """A CategoryIndex over this model's items, or over an ItemScope's (within=), by the model's item_cate."""
        return CategoryIndex(self.item_cate, self.config["cate_count"], self.device,
                             within=scope_within(within, self.config["item_count"]))

    def cluster_index(self, nlists, within=None, iters=10, seed=1234, train_size=None, max_list=None):
        """A ClusteredIndex (cluster.py) over this model's items, or over an ItemScope's (within=): nlists lists learned by
        k-means from the item vectors as stored -- the `index=` that goes with `probes=` in recommend and similar_items.
        A snapshot of the parameters: rebuild it after training."""
        from .cluster import fit
        return fit(self, nlists, within=within, iters=iters, seed=seed, train_size=train_size, max_list=max_list)

    def shortlist_index(self):
        """A ShortlistIndex (shortlist.py) over this model's items: the bf16 snapshot of the item vectors as stored and the
        largest row norm -- the `index=` behind recommend's two-stage exact lists.  A snapshot of the parameters: rebuild
        it after training."""
        from .shortlist import build
        return build(self)

    def recommend(self, batch, k, exclude=None, diversity=0.0, per_category=0, pool=None, within=None, category=None, index=None,
                  probes=None, shortlist=None, fallback=True, boost=None, boost_weight=None, after=None):
        """The k best items over ALL items for each row -- what tf.nn.top_k(eval_logits, k) gives the reference
        (model.py:140) -- without materialising the [B, I] scores.  Takes label_ranks' batches (the label and the
        negative are not used).  -> (ids [B, k] int32, scores [B, k] float32) device tensors, in tf.nn.top_k's
        order (higher score first, ties -> lower id); rows with fewer than k eligible items end in -1 / -inf.
        exclude: None; "history" -- the items the row's input holds (the last Ls items and the current session);
        a sequence of B arrays of item ids; or a SeenItems holder -- the user's seen items and the row's input.  Scores equal label_ranks' / eval_label_scores' bit for bit.
        diversity (theta in [0, 1]), per_category (m >= 0; 0 = no cap), pool: a second stage over
        the row's N = pool (default min(256, max(4 k, 32)); k <= N <= 256) best items, tlsan_rerank.  Valid pool entries
        (id >= 0, finite score) get the relevance r_j = (s_j - s_lo) / (s_hi - s_lo) over the pool's first / last valid
        score (0 when equal) and the list is picked greedily: an entry is eligible while it is not selected and (m > 0)
        fewer than m selected entries share its category; its value is (1 - theta) r_j for the first pick, afterwards
        (1 - theta) r_j - theta * max over the selected i of cos(i, j), the cosine of similar_items; the largest value
        wins, equal values -> higher in the pool; when nobody is eligible the row ends in -1 / -inf.  The scores
        returned are the model's own, bit for bit, in selection order.  theta = 0 with m > 0 is exact whenever the row
        comes back full: it is the capped ranking over ALL eligible items (the pool is the exact score-order prefix); a
        short row means the pool was too small -- raise it.  With both left at 0 nothing changes: the plain top-k path,
        the same launches and bits (pool alone is a ValueError).
        within (an ItemScope) / category ([B] category ids, array or tensor; -1: the row is unrestricted; an id >=
        cate_count is a ValueError): the k best WITHIN the scope's items and, per row, within that category
        (last_item_categories gives "the department the row is in") -- tlsan_eval_topk_scoped.  Only the scope's items
        are scored, so a list costs what a table of within.count items costs; the category-only form still scans the
        whole table, or the scope.  Same scores, bit for bit, as without them; both compose with
        exclude= and with diversity / per_category / pool (the scoped list is the pool).  With both None the old entry
        point runs: the same launches and bits.  label_ranks takes no scope.
        index (a CategoryIndex, category_index()): a row scores the lists of the categories it asks for and nothing
        else -- tlsan_eval_topk_lists; the same ids and score bits as the category form without it.  category is then
        required, [B] or [B, P] with P <= 8: a row gets the best of the UNION of its categories (a negative entry is no
        probe, a repeated id counts once); a row of negatives only is unrestricted and runs through the path without
        an index as a sub-batch (one host read finds such rows).  The scope belongs to the index
        (category_index(within=scope)): within= beside index= is a ValueError, as are an index over another item or
        category count, an id >= cate_count, P > 8 and a wrong shape, all before any launch.  exclude= and the second
        stage compose as with the scope: the indexed list is the pool.  Worth it when a category is a small part of
        the table (profiles/category_index.md); with index=None nothing changes.
        index (a ClusteredIndex, cluster_index()) with probes=P, 1 <= P <= 64: an APPROXIMATE list over the whole
        catalogue (or the index's scope) -- the row scores the P lists whose centroids score highest against it
        (tlsan_cluster_probe, with the table scale and the lists' mean bias) and nothing else: tlsan_eval_topk_lists on
        groups of 8 probes, merged.  Every returned score is the exact path's bit for bit and the list is the exact top k
        of the probed lists' union minus the exclusions; with P >= the number of non-empty lists it equals recommend()
        without an index.  Recall at fewer probes is not guaranteed (cluster.recall measures it).  category= or within=
        beside it, probes= without it or outside 1..64, or an index over another item count: ValueError before any launch.
        index (a ShortlistIndex, shortlist_index()) with shortlist=N (default min(256, max(4 n, 64)), n the list length
        asked of the first stage: k, or the diversity pool; n < N <= 256): the EXACT list over the whole catalogue in two
        stages -- the N best by bf16 score (tlsan_shortlist_topk), their exact scores (tlsan_score_candidates), the n best
        of those and, per row, a certificate that no item outside the shortlist can belong to the exact list
        (tlsan_shortlist_select).  fallback=True: the rows without a certificate (one host read finds them) run through
        the path without an index as a sub-batch, so every row is recommend()'s without an index, ids and score bits;
        fallback=False: the shortlist's lists as they are.  index.certified is the call's [B] bool device tensor,
        index.counts the (rows, certified) of all calls.  exclude= and the second stage compose; within=, category= or
        probes= beside it, shortlist= without it, n >= N, or an index over another item count or d: ValueError before any
        launch.
        boost (an ItemBoost, item_boost(); or an array or tensor of item_count values, wrapped) / boost_weight ([B]
        numbers, array or tensor): every score becomes s' = fl(s + boost[g]), or fl(s + fl(boost_weight[b] * boost[g]))
        with weights (fp32, separate roundings), INSIDE the selection -- tlsan_eval_topk_scoped_boost /
        tlsan_eval_topk_lists_boost -- so a promoted item just outside the unboosted list is found.  Selection, ties
        (lower id), zeros and NaN (last) follow s'; the scores returned are s' (score_candidates on the ids gives the raw
        ones).  -inf buries an item behind every finite score but does not remove it: exclude= / within= remove items.  An
        all-zero boost, or a weight of 0, gives the unboosted row, ids and bits.  It composes with exclude=, within=,
        category=, a CategoryIndex (the unrestricted sub-batch carries the boost and its rows' weights), a ClusteredIndex
        (probing still picks the lists by the UNBOOSTED centroid scores; probing every non-empty list is the boosted
        exact result) and the second stage (the pool is the boosted list and the relevance is formed from s').  With both
        None nothing changes: the same launches and bits.  boost_weight without boost, a boost over another item count,
        a weight of the wrong length, or boost= beside a ShortlistIndex (its certificate bounds the model's score, not
        s'): ValueError before any launch.  similar_items, audience and label_ranks take no boost.
        after (a ListCursor, ListCursor.of(ids, scores) of the page before; or an (ids, scores) pair of [B] arrays or
        tensors, wrapped): the NEXT k entries of the same call's ranking -- a row selects only what the call without
        after= ranks strictly behind its cursor (by s' when boosted), so pages chained through their last columns tile
        the exact ranking, ids and score bits, at any depth and for one scan a page: k stays 1..256, the depth does not.
        Rows may sit at different depths: ListCursor.START (-2) is no cursor, the page after a short page is empty and
        stays empty (cursor.done).  The cursor is a position, not an item: it need not be in the scope or eligible.  It
        composes with exclude=, within=, category=, boost= / boost_weight= (tlsan_eval_topk_scoped_after), a
        CategoryIndex (the unrestricted sub-batch carries its rows' cursors) and a ClusteredIndex (the probe sees u_t
        alone, so every page probes the same lists and the pages tile the ranking of the probed union) --
        tlsan_eval_topk_lists_after.  A cursor is a snapshot: pages tile only while parameters, boost, scope and
        exclusions stay the same; nothing detects a change.  With None nothing changes: the same launches and bits.
        after= beside diversity / per_category / pool (the greedy second stage is not a prefix order) or a
        ShortlistIndex (its first stage ranks by bf16 score and its certificate is about the head of the list), a
        cursor of another length than the batch, or one that cannot be converted: ValueError before any launch.
        recommend_deep chains the pages on the device.  shelves, similar_items, label_ranks and explain take none."""
        after = None if after is None else cursor_of(after, batch_rows(batch), self.device)
        topk, N, db = self._recommend_lists(batch, k, after is not None, exclude=exclude, diversity=diversity,
                                            per_category=per_category, pool=pool, within=within, category=category, index=index,
                                            probes=probes, shortlist=shortlist, fallback=fallback, boost=boost,
                                            boost_weight=boost_weight)
        if N is None:
            return topk(k, after)
        # (forward has landed an owed lazy-L2 correction; the vectors are read as stored, the scale not folded)
        st = self._stream()
        pid, psc = topk(N, None)
        ids = torch.empty(db.B, int(k), dtype=torch.int32, device=self.device)
        scores = torch.empty(db.B, int(k), dtype=torch.float32, device=self.device)
        rows = rerank_chunk(N, self.config["hidden_units"])
        for r0 in range(0, db.B, rows):
            flat = pid[r0:r0 + rows].reshape(-1)
            vec, inv = item_vectors(self.lib, self.dims, self.cparams, flat, 1, 0, st)
            cate = self.item_cate[flat.clamp(min=0).long()]
            rerank(self.lib, pid[r0:r0 + rows], psc[r0:r0 + rows], vec, inv, cate, k, diversity, per_category,
                   ids[r0:r0 + rows], scores[r0:r0 + rows], st)
        return ids, scores

    def recommend_deep(self, batch, n, page=256, **kw):
        """The n best items of each row for ANY n >= 1 -- recommend(batch, n, **kw) without its limit of 256 -- in
        ceil(n / page) scans of `page` entries (1..256) behind ONE forward: the pages' cursors are chained on the device
        (ListCursor.of's columns), no host read between them.  -> (ids [B, n] int32, scores [B, n] float32), the exact
        ranking, ids and score bits; rows with fewer than n eligible items end in -1 / -inf.  kw: recommend's exclude=,
        within=, category=, index= (a CategoryIndex or a ClusteredIndex with probes=), boost=, boost_weight= and after= (a
        cursor to start behind); what recommend refuses beside after= is refused here."""
        n, page = check_deep(n, page)
        after = kw.pop("after", None)
        after = None if after is None else cursor_of(after, batch_rows(batch), self.device)
        topk, _, _ = self._recommend_lists(batch, page, True, **kw)
        return deep_pages(topk, n, page, after)

    def _recommend_lists(self, batch, k, paged, exclude=None, diversity=0.0, per_category=0, pool=None, within=None, category=None,
                         index=None, probes=None, shortlist=None, fallback=True, boost=None, boost_weight=None):
        """What recommend and recommend_deep share: recommend's argument checks (paged: the call takes a cursor, so the
        second stage and a ShortlistIndex are refused), one forward and the exclusion lists -> (topk, N, db) with
        topk(n, after) the call's lists of n entries behind the ListCursor `after` (None: the entry points without a
        cursor, as ever) and N the second stage's pool size or None."""
        from .cluster import clustered_probes, clustered_topk
        from .shortlist import ShortlistIndex, shortlist_size, shortlist_topk
        N = rerank_pool(k, diversity, per_category, pool)
        if paged and N is not None:
            raise ValueError("after= beside diversity / per_category / pool: the greedy second stage is not a prefix order")
        if paged and isinstance(index, ShortlistIndex):
            raise ValueError("after= beside a ShortlistIndex: its first stage ranks by bf16 score and its certificate is about the "
                             "head of the list")
        short = shortlist_size(index, shortlist, int(k) if N is None else N, self.config["item_count"], self.config["hidden_units"],
                               category=category, within=within, probes=probes)
        probes = None if short is not None else clustered_probes(index, probes, self.config["item_count"], category=category, within=within)
        within = scope_within(within, self.config["item_count"])
        boost = boost_of(boost, boost_weight, batch_rows(batch), self.config["item_count"], self.device)
        if boost is not None and short is not None:
            raise ValueError("boost= beside a ShortlistIndex: its certificate bounds the model's score, not the boosted one")
        if probes is not None or short is not None:
            pass
        elif recommend_index(index, within, self.config["item_count"], self.config["cate_count"]) is not None:
            category = index_categories(category, batch_rows(batch), self.config["cate_count"], self.device)
        else:
            category = scope_categories(category, batch_rows(batch), self.config["cate_count"], self.device)
        _, _, ut, db = self.forward(batch, is_test=True, want_u_t=True)
        excl, st = exclusion_csr(db, exclude, self.config["item_count"]), self._stream()
        if short is not None:
            topk = lambda n, after: shortlist_topk(self.lib, self.dims, self.cparams, ut, db.B, n, excl, index, short, fallback,
                                            self._topk_workspace, st)
        elif probes is not None:
            topk = lambda n, after: clustered_topk(self.lib, self.dims, self.cparams, ut, db.B, n, excl, index, probes,
                                                   self._scale_vector(index.lists), self._topk_workspace, st, boost=boost, after=after)
        elif index is not None:
            found = {}      # (the unrestricted rows: read from the device once, by the first page)
            topk = lambda n, after: indexed_topk(self.lib, self.dims, self.cparams, ut, db.B, n, excl, index, category, 1, 0,
                                                 self.config["item_count"], self._topk_workspace, st, boost=boost, after=after,
                                                 found=found)
        elif within is None and category is None and boost is None:
            # (the plain path keeps tlsan_eval_topk; behind a cursor it is the scoped call over the whole table)
            topk = lambda n, after: (eval_topk(self.lib, self.dims, self.cparams, ut, db.B, n, excl, 1, 0, self._topk_workspace, st)
                                     if after is None else
                                     scoped_topk(self.lib, self.dims, self.cparams, ut, db.B, n, excl, None, None, 1, 0,
                                                 self._topk_workspace, st, after=after))
        else:
            sub = None if within is None else within.sub(1, 0, self.config["item_count"])
            topk = lambda n, after: scoped_topk(self.lib, self.dims, self.cparams, ut, db.B, n, excl, sub, category, 1, 0,
                                                self._topk_workspace, st, boost=boost, after=after)
        return topk, N, db

    def shelves(self, batch, shelves, k, index=None, exclude=None, min_items=1, rank_at=0, skip=None, seg_items=None,
                big_items=None):
        """A page of category shelves for each row: its S = shelves best categories and the m = k best items of each, in
        one scan of the index -> (cats [B, S] int32, ids [B, S, m] int32, scores [B, S, m] float32) device tensors
        (tlsan_eval_shelves).  Takes recommend's batches.
        index (a CategoryIndex, category_index()) is required; its scope is the page's: category_index(within=scope)
        removes items, and a category the scope empties is never a shelf.  exclude is recommend's: None, "history", B id
        lists or a SeenItems.  skip: None, [B] or [B, X] category ids, X <= 8 (array or tensor; negative: nothing) that are
        not offered as shelves for that row -- last_item_categories gives "not the department the row is already in".
        For row b and category c, L(b, c) is row b of recommend(batch, m, exclude=exclude, category=np.full(B, c),
        index=index), ids and score bits, and n(b, c) its valid entries.  Category c is a candidate of row b when it is
        not skipped and n(b, c) >= min_items (1 <= min_items <= m); its rank key is entry rank_at of L(b, c) (0 <= rank_at
        < min_items, so the entry exists): rank_at=0 ranks a department by its best item, rank_at=min_items-1 by the
        weakest item it is sure to show.  No arithmetic is done on scores: the order of shelves is recommend's order of
        those entries (higher score first, equal scores -> lower item id, NaN last).  The page is the S candidates of
        highest rank key in that order; a row with fewer ends in cats -1, ids -1, scores -inf, and a shelf's entries past
        n(b, c) are -1 / -inf.  ids.view(B, S * m) is a list list_metrics takes.
        Limits: 1 <= S <= 32, 1 <= m <= 64, S * m <= 256.  A breach, rank_at >= min_items, min_items > m, a missing index
        or one over another item or category count, a skip of the wrong shape or with an id >= cate_count: ValueError
        before any launch.  Out of scope, and not arguments: boost=, diversity / per_category, within= (the scope belongs
        to the index) and category= (skip= says which categories not to offer).
        seg_items / big_items: the thresholds of the scan's plan (shelves_plan; None: shelves_thresholds' production
        values).  They decide the launch geometry, never the result; the plan is cached on the index.  The result is a
        function of (row, index, arguments): not of the batch, the row order or a repeated call.  Nothing in the model
        changes; every other call keeps its launches and bits."""
        I, Cn = self.config["item_count"], self.config["cate_count"]
        S, m, min_items, rank_at = shelves_sizes(shelves, k, min_items, rank_at)
        index = shelves_index(index, I, Cn)
        skip = shelves_skip(skip, batch_rows(batch), Cn, self.device)
        _, _, ut, db = self.forward(batch, is_test=True, want_u_t=True)
        excl, st = exclusion_csr(db, exclude, I), self._stream()
        dflt = shelves_thresholds(index.count, db.B)
        plan = index.shelf_plan(1, 0, I, dflt[0] if seg_items is None else seg_items, dflt[1] if big_items is None else big_items)
        return shelves_topk(self.lib, self.dims, self.cparams, ut, db.B, S, m, min_items, rank_at, excl, index.local(1, 0, I), skip,
                            1, 0, self._topk_workspace, st, plan=plan)

    def list_metrics(self, ids, labels=None, item_weight=None, exposure=None):
        """What the lists ids [B, K] (tensor or array of global item ids, -1 = no entry, anywhere; 1 <= K <= 256; for
        instance what recommend returned) look like beside their accuracy -> ListMetrics, [B] device tensors
        (tlsan_list_metrics): valid entries, summed pairwise cosines (similar_items' / recommend's cosine of
        [item_emb || cate_emb[item_cate]]) and the intra-list diversity ILD, distinct categories and the most entries
        sharing one (<= m for a list made with per_category=m), the position of labels [B] (None: -1 everywhere) and the
        summed item_weight [item_count] of the entries (the novelty hook: input.item_self_information).  exposure: a
        [item_count] int32 device counter; every valid entry adds 1 to its item's (never cleared here).  Rows go through
        in rerank_chunk pieces, staged as recommend's second stage stages them.  Like similar_items it reads the tables as
        stored: an owed lazy-L2 correction lands first, the scale is NOT folded -- parameters, scale and state keep their
        bits.  A wrong shape, K outside 1..256 or an id >= item_count is a ValueError before any launch."""
        ids, labels, item_weight = list_metric_inputs(ids, labels, item_weight, exposure, self.config["item_count"], self.device)
        self._flush()
        st = self._stream()

        def measure(sub, lab):
            flat = sub.reshape(-1)
            vec, inv = item_vectors(self.lib, self.dims, self.cparams, flat, 1, 0, st)
            g = flat.clamp(min=0).long()
            return list_metrics(self.lib, sub, vec, inv, self.item_cate[g], lab,
                                None if item_weight is None else item_weight[g], exposure, st)
        return list_metrics_chunks(ids, labels, rerank_chunk(ids.shape[1], self.config["hidden_units"]), measure)

    def _scale_vector(self, n):
        """The table scale as the probe takes it: [n] float32 on the device, read from the state without a host round
        trip; None where there is no scale (dense L2: 1)."""
        if self.l2_mode != L.L2_LAZY:
            return None
        return self.state[:4].view(torch.float32).expand(n).contiguous()

    def similar_items(self, items, k, metric="cosine", exclude=None, within=None, same_category=False, index=None, probes=None):
        """The k nearest items of each item of `items` (a 1-D list, array or tensor of global ids; outside
        [0, item_count): ValueError) by the representation the model scores with, [item_emb || cate_emb[item_cate]]:
        metric "cosine" or "dot" (the product of the true vectors: the table scale enters twice); no bias, no user.
        -> (ids [Q, k] int32, scores [Q, k] float32) device tensors in recommend's order; the query never appears in
        its own list, nor do the items of exclude (None, or a sequence of Q id sequences); rows with fewer than k
        eligible items end in -1 / -inf.  Selected inside the scoring kernel (tlsan_similar_topk): the [Q, I]
        similarities are never materialised.  Reads the tables as they are stored: an owed lazy-L2 correction lands
        first, the scale is NOT folded -- parameters, scale and state keep their bits.
        within (an ItemScope): the nearest WITHIN the scope's items, of which alone the similarities are formed;
        same_category: query q's list holds items of item_cate[q]'s category only (it still scans the scope, or the
        whole table without one) -- tlsan_similar_topk_scoped, same score bits.  With neither the old entry point runs.
        index (a CategoryIndex) with same_category=True: query q scores the list of item_cate[q] and nothing else
        (tlsan_similar_topk_lists), same ids and score bits; index= without same_category=True, or beside within=
        (the scope belongs to the index), is a ValueError.
        index (a ClusteredIndex) with probes=P: the approximate form, as in recommend -- the query's vector picks its P
        lists (cosine: against the normalised centroids; dot: the plain product; no bias), tlsan_similar_topk_lists on
        groups of 8, merged; same_category= or within= beside it is a ValueError."""
        from .cluster import clustered_probes, clustered_similar_topk
        qids, mc, excl = similar_queries(items, self.config["item_count"], metric, exclude, self.device)
        probes = clustered_probes(index, probes, self.config["item_count"], same_category=same_category, within=within)
        within = scope_within(within, self.config["item_count"])
        if probes is None:
            index = similar_index(index, within, same_category, self.config["item_count"], self.config["cate_count"])
        self._flush()
        st = self._stream()
        vec, inv = item_vectors(self.lib, self.dims, self.cparams, qids, 1, 0, st)
        if probes is not None:
            return clustered_similar_topk(self.lib, self.dims, self.cparams, vec, inv, qids, k, mc, excl, index, probes,
                                          self._topk_workspace, st)
        if index is not None:
            cate = self.item_cate[qids.long()].to(torch.int32).reshape(-1, 1).contiguous()
            return lists_similar_topk(self.lib, self.dims, self.cparams, vec, inv, qids, k, mc, excl,
                                      index.local(1, 0, self.config["item_count"]), cate, 1, 0, self._topk_workspace, st)
        if within is None and not same_category:
            return similar_topk(self.lib, self.dims, self.cparams, vec, inv, qids, k, mc, excl, 1, 0, self._topk_workspace, st)
        sub = None if within is None else within.sub(1, 0, self.config["item_count"])
        cate = self.item_cate[qids.long()].to(torch.int32).contiguous() if same_category else None
        return scoped_similar_topk(self.lib, self.dims, self.cparams, vec, inv, qids, k, mc, excl, sub, cate, 1, 0,
                                   self._topk_workspace, st)

    def user_vectors(self, batches, real=None):
        """The rows' u_t as a UserVectors: `batches` is one test-style batch (a tuple or a DeviceBatch, whatever recommend
        takes) or an iterable of them; each goes through forward(is_test=True, want_u_t=True) and the rows are
        concatenated in the order given.  A row is a sample -- a user at a point of their history; the test set has one
        row per user.  real (None, or one count per batch): only a batch's first real rows are kept (a padded launch).
        A snapshot of the parameters: rebuild it after training."""
        batches = batch_list(batches)
        real = kept_rows(real, len(batches))
        vec, user = [], []
        for batch, n in zip(batches, real):
            _, _, ut, db = self.forward(batch, is_test=True, want_u_t=True)
            vec.append(ut[:n])
            user.append(db.u[:n])
        if not vec:
            raise ValueError("user_vectors: no batch given")
        return UserVectors(torch.cat(vec), torch.cat(user), self, self._step)

    def audience(self, items, k, users, exclude=None, after=None):
        """The k best ROWS of `users` (a UserVectors of this model at its current global step) for each item of `items` (a
        1-D list, array or tensor of global ids, repeats allowed; outside [0, item_count): ValueError): whom to notify
        about an item.  -> (rows [Q, k] int32, scores [Q, k] float32) device tensors in recommend's order (higher score
        first, ties -> lower row); users.users_of(rows) gives the user ids; with fewer than k eligible rows a list ends in
        -1 / -inf.  A row appears with exactly the score the item has in that row's recommend / score_candidates list,
        bit for bit: tlsan_dense_topk runs recommend's tiles with the item's stored vector in u_t's place, the table
        scale and the item's item_b applied as recommend applies them; the [N, Q] scores are never materialised.
        exclude: None; a sequence of Q sequences of global row numbers; or a SeenItems holder -- every row whose user
        has item q in their seen list stays out of q's list (seen_rows_csr).  The item side is read at call time, as
        similar_items reads it: an owed lazy-L2 correction lands first, the scale is NOT folded -- parameters, scale and
        state keep their bits.  k outside 1..256, or users that are not this model's at this step (another model,
        another d or device, trained since): ValueError before any launch.
        after (a ListCursor over the Q query items, in global ROW numbers; or an (ids, scores) pair, wrapped): the next k
        rows of each item's audience, strictly behind its cursor -- recommend's after=, on tlsan_dense_topk_after: pages
        chained through ListCursor.of tile the exact audience at any depth (a notification batch of thousands), ids and
        score bits; ListCursor.START is no cursor, the page after a short page is empty.  A snapshot, as `users` is.  A
        cursor of another length than items: ValueError before any launch.  audience_deep chains the pages."""
        topk, after = self._audience_lists(items, k, users, exclude, after)
        return topk(k, after)

    def audience_deep(self, items, n, users, page=256, exclude=None, after=None):
        """The n best rows of `users` for each item for ANY n >= 1 -- audience(items, n, users) without its limit of 256
        -- in ceil(n / page) scans of `page` rows (1..256) behind ONE read of the items' vectors; the pages' cursors are
        chained on the device, no host read between them.  -> (rows [Q, n] int32, scores [Q, n] float32), the exact
        ranking, ids and score bits; exclude= and after= are audience's."""
        n, page = check_deep(n, page)
        topk, after = self._audience_lists(items, page, users, exclude, after)
        return deep_pages(topk, n, page, after)

    def _audience_lists(self, items, k, users, exclude, after):
        """What audience and audience_deep share: the checks, the exclusion lists and one tlsan_item_vectors -> (topk, the
        checked cursor): topk(k, after) the queries' lists of k rows behind the ListCursor `after` (None: tlsan_dense_topk,
        as ever)."""
        qids = audience_queries(items, k, self.config["item_count"], self.device)
        after = cursor_of(after, int(qids.shape[0]), self.device)
        check_user_vectors(users, self, self._step, self.config["hidden_units"], self.device)
        if len(users) < 1:
            raise ValueError("users: no rows")
        excl = audience_exclusion(exclude, qids, users)
        self._flush()
        st = self._stream()
        vec, _ = item_vectors(self.lib, self.dims, self.cparams, qids, 1, 0, st)
        scale, bias = self._scale_vector(int(qids.shape[0])), self.item_b[qids.long()].contiguous()
        return (lambda k, after: dense_topk(self.lib, vec, users.vec, scale, bias, excl, 0, k, self._topk_workspace, st, after=after)), after

    def score_candidates(self, batch, candidates):
        """Scores of caller-given items: candidates [B, C] global item ids (array or tensor; -1 = padding, which scores
        -inf) -> [B, C] float32 device tensor, u_t[b] . [item_emb || cate_emb[item_cate]][g] + item_b[g].  A score
        equals label_ranks' / recommend's for the same (row, item) bit for bit."""
        _, _, ut, db = self.forward(batch, is_test=True, want_u_t=True)
        cand = candidate_tensor(candidates, db.B, self.device)
        return score_candidates(self.lib, self.dims, self.cparams, ut, cand, 1, 0, self._stream())

    def explain(self, batch, items, top=3, by="item", order="positive", parts=False):
        """Why these items: the exact parts of the score of every (row, item) of items [B, Kc] (array or device tensor of
        global ids, typically recommend's ids; a negative id -- recommend's -1 tail -- is padding) -> Explanation.  Takes
        recommend's batches.  The score is linear in everything behind the two softmaxes, so with the attention weights
        of the row's forward (forward(want_att=True): att0 / att1 stay on the model) it splits exactly into a bias, a
        user part, the bridge's offset and one part per position of the long window and of the session
        (tlsan_explain, include/tlsan.h); the parts of a row add up to score_candidates' score up to
        fp32 rounding.
        top (1..16): the strongest history sources of every (row, item), selected in the kernel -- Explanation.src /
        .item / .value / .kind.  by="item": the positions of a row that hold the same item id are one source (their
        parts summed), "position": every valid position is one.  order="positive": the largest part first ("because you
        viewed X"), "abs": the largest magnitude first.  Ties go to the earlier column, NaN last.
        parts=True: also the [B, Kc, 3 + Ls + Sn] parts themselves (Explanation.columns names them); without it no such
        array exists anywhere and the selection is the same bit for bit.
        The parts decompose the fp32 model: with matrix_dtype="bf16" they are those of the fp32 score under the bf16
        forward's attention weights.  A wrong shape, top outside 1..16, an unknown by or order: ValueError before any
        launch; an id >= item_count, and a batch of more than 192
        positions per row (Ls + Sn: the selection is quadratic in them), is refused by the library before its launch.  Nothing in the model changes."""
        r, cby, corder = explain_args(top, by, order)
        cand = candidate_tensor(items, batch_rows(batch), self.device)
        _, _, _, db = self.forward(batch, is_test=True, want_att=True)
        return explain(self.lib, self.dims, self.cparams, db, self.att0, self.att1, cand, r, cby, corder, bool(parts), self._stream())

    def sample_negatives(self, batch, n, seed=1234, row0=0, exclude="history"):
        """n distinct negatives per row -> [B, n] int32 device tensor (-1 where fewer are found): the first n eligible
        items of row (row0 + b)'s draw sequence under `seed` (tlsan_sample_negatives; never the label, never an item
        of `exclude`, which takes recommend's forms).  Depends on (seed, row0 + b, label, exclusion, n) only."""
        db = self.device_batch(batch, is_test=True)
        return sample_negatives(self.lib, self.config["item_count"], db.i, n, seed, row0,
                                exclusion_csr(db, exclude, self.config["item_count"]), self._stream())

    def sampled_ranks(self, batch, n, seed=1234, row0=0, exclude="history"):
        """Rank of each row's label among its n sampled negatives (sample_negatives) -> [B] int32 device tensor: one
        forward, one sampling, one scoring of [label | negatives], one ranking; no host round trip."""
        _, _, ut, db = self.forward(batch, is_test=True, want_u_t=True)
        st = self._stream()
        score = lambda ut, cand: score_candidates(self.lib, self.dims, self.cparams, ut, cand, 1, 0, st)
        return sampled_ranks(self.lib, self.config["item_count"], db, ut, n, seed, row0, exclude, score, st)

    def _topk_workspace(self, nbytes):
        return grow_workspace(self, "_tws", nbytes)

    def check_static_overflow(self):
        """ShardedModel's check of its fixed-size exchanges, which the driver makes before an evaluation: none here."""

    def _hits(self, batch, ranks=None):
        h = hits_and_rows(self.label_ranks(batch) if ranks is None else ranks)
        return h[:-1], int(h[-1])

    def eval_prec(self, sess, batch, ranks=None):
        """Streaming precision_at_k update ops (model.py:265-281); counters are cumulative over
        every call, like the reference's never-reset local variables (train.py:75-76,82).
        ranks (optional): the label ranks of this batch's rows, already computed (label_ranks on a larger launch)."""
        return self._topk.add_prec(*self._hits(batch, ranks))

    def eval_recall(self, sess, batch, ranks=None):
        return self._topk.add_recall(*self._hits(batch, ranks))

    def reset_metrics(self):
        """Not in the reference (its counters are never reset); provided for per-round metrics."""
        self._topk.reset()

    # ------------------------------------------------------------------ checkpoint
    def save(self, sess=None):
        """model.py:302-307: parameters + config JSON next to them."""
        os.makedirs(self.config["model_dir"], exist_ok=True)
        base = os.path.join(self.config["model_dir"], "TLSAN")
        path = "%s-%d.npz" % (base, self._step)
        write_checkpoint(path, self._step, self._epoch, self.get_params(), self.get_slots())
        json.dump(self.config, open("%s-%d.json" % (base, self._step), "w"), indent=2)
        if not self.config.get("quiet"):
            print("model saved at %s" % path, flush=True)
        return path

    def restore(self, sess, path):
        """model.py:310-313."""
        step, epoch, params, slots = read_checkpoint(path, want_slots=self.slots is not None)
        if slots is not None:
            self._check_slots(slots)      # (another optimizer's checkpoint: refused before anything is loaded)
        self.set_params(params)
        self._step, self._epoch = step, epoch
        if slots is not None:
            self.set_slots(slots)
        if not self.config.get("quiet"):
            print("model restored from %s" % path, flush=True)

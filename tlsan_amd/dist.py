"""Multi-GPU TLSAN step: one process per GPU, embedding tables row-sharded, RCCL over xGMI.

The reference is single-GPU (train.py:53,146); this is the MI355X-native scale-out of
SURVEY.md section 8e.  Samples are independent units: every rank trains its own batch
(data parallel, weak scaling).  State placement:

  * ``user_emb`` + ``usert_emb`` rows: sharded by ``user_id % world``  (fused rows
    ``[user_emb | usert_emb | pad]``);
  * ``item_emb`` + ``item_b`` rows: sharded by ``item_id % world`` (fused ``[item_emb | item_b | pad]``;
    mod-G spreads the Zipf-hot items);
  * ``cate_emb`` (<= 5 MB), ``item_cate_list`` and the dense attention weights: replicated.

This module holds ``ShardedModel``: the parameters, their checkpoints, gather / scatter and the evaluation surface.  The
training step -- its phases and collectives, in the form whose exchange sizes pass through the host and in the
static-shape form -- is described and lives in ``tlsan_amd.dist_step``; the collectives and the key space of the routing
in ``tlsan_amd.dist_comm`` (re-exported here).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib as L
from .dist_comm import (ExchangePlan, KeyRouter, ModPartition, RowExchange, _staged, a2a, allgather_rows,  # noqa: F401
                        allreduce_sum, torch_scan)
from .shortlist import ShortlistIndex
from .dist_step import DynamicStep, FlatLayout, StaticStep, fused_params
from .model import (LAZY_ADAGRAD_OPTIMIZERS, LAZY_OPTIMIZERS, OPTIMIZERS, DeviceBatch, Model, TopKCounters, _Var, _Writer, candidate_tensor, eval_topk,
                    exclusion_csr, grow_workspace, hits_and_rows, pack_dense, read_checkpoint, sample_negatives, sampled_ranks,
                    score_candidates, item_vectors, list_metric_inputs, list_metrics, list_metrics_chunks, rerank, rerank_chunk, rerank_pool, batch_rows, last_items, scope_categories, scope_within, scoped_similar_topk, scoped_topk, CategoryIndex, index_categories, indexed_topk, recommend_index, lists_similar_topk, similar_index, similar_queries, similar_topk, topk_merge, ItemScope, boost_of, item_boost_for, unpack_dense, write_checkpoint,
                    UserVectors, audience_exclusion, audience_queries, batch_list, check_user_vectors, dense_topk, kept_rows,
                    ListCursor, check_deep, cursor_of, deep_pages)


def _ru4(x):
    return (x + 3) // 4 * 4


def refuse_clustered(index, probes=None):
    """A ClusteredIndex (or its probes=) beside a ShardedModel: a ValueError before anything is gathered or launched."""
    from .cluster import ClusteredIndex
    if isinstance(index, ClusteredIndex) or probes is not None:
        raise ValueError("ShardedModel: a ClusteredIndex is not supported on a row-sharded model (building and probing "
                         "across ranks); use a CategoryIndex, or a Model")


class ShardedModel:
    """Model surface (train / eval_auc / ...) over row-sharded tables; see module docstring."""

    def __init__(self, config, item_cate_list, device="cuda:0", seed=1234, group=None, l2_mode="dense", static_rows=False,
                 wire_dtype="f32", init="numpy", deferred_ids=False, coalesce=False):
        """l2_mode: "dense" -- every owner decays every one of its rows every step, as the reference's dense L2
        gradient does; "lazy" (sgd) -- the same update kept as W = P * W_stored with one scale P that all ranks
        advance alike, so an owner touches only the rows whose gradients arrived (tlsan_shard_apply_lazy); with
        config["optimizer"] "lazy_adam" / "lazy_rmsprop" / "lazy_adadelta" (which need l2_mode="lazy") -- the dense optimizer's
        step restricted to the rows the GLOBAL batch used (tlsan_shard_apply_lazy_opt): the item and user rows that reached
        their owner, and the category rows some rank's batch used (a use flag per category rides in the step's all-reduce, so
        every rank decides alike); every other row keeps its value and both accumulators bit for bit, the dense weights move
        every step, loss and clip norm are the dense optimizer's, and the table scale stays 1.  The lazy optimizers have no
        static-shape step: static_rows (and with it graph capture and wire_dtype="bf16") is refused for them.
          wire_dtype (static_rows only): "f32", or "bf16" -- rows cross the wire with bf16 embedding values (fp32 weights
        stay with their owners; see below).
          static_rows (lazy only): False -- exchange sizes follow the batch (the host reads them once per step);
        True or an int -- every (source, owner) pair exchanges a FIXED number of row slots (the int, or 1.5 x what
        the first batch needs, agreed over the ranks), no size reaches the host, and a step can be recorded in a HIP
        graph (capture_step / replay).  A batch that needs more slots than that raises at the next host check.
          deferred_ids (static_rows): plans built ahead never carry their own id all-to-all -- the step that uses a plan
        issues it, on the main stream -- which is what runs by default over RCCL (no second communicator); True forces
        the same under the gloo exchange of the tests, whose default keeps a side group.
          coalesce (static_rows): the all-reduce of the dense gradients and the all-to-all of the row gradients, which do
        not depend on each other, are issued as ONE RCCL group (one launch, one latency) ahead of the summary -- the row
        gradients then travel BEFORE the clip coefficient exists (unscaled; the coefficient reaches the owners through the
        summary).  Under the gloo exchange of the tests the group is two staged calls back to back: the ORDER of the
        phases of the step, which is what differs from the default, is covered by the two-process tests
        (tests/test_gpu_shard_static.py); the RCCL group itself only where there are two GPUs (tests/test_gpu_configs.py).
        Off by default: no hardware with more than one GPU has ever run it."""
        if l2_mode not in ("dense", "lazy"):
            raise ValueError("l2_mode must be 'dense' or 'lazy'")
        self.lazy = l2_mode == "lazy"
        if static_rows and not self.lazy:
            raise NotImplementedError("static_rows is the lazy-L2 step's form (l2_mode='lazy')")
        if wire_dtype not in ("f32", "bf16"):
            raise ValueError("wire_dtype must be 'f32' or 'bf16'")
        if wire_dtype == "bf16" and not static_rows:
            raise NotImplementedError("wire_dtype='bf16' is built for the static-shape step (static_rows)")
        # wire_dtype="bf16": the owners keep (and update) fp32 rows; the copies that travel to the ranks using them, and
        # that the kernels gather from, carry the embedding values as bf16 (round to nearest even) -- 176 instead of 304
        # bytes per row at d = 128, Ls = 10.  The category table (replicated) is read through a bf16 shadow refreshed
        # every step.  Gradients travel back in fp32.
        self.wire_dtype = wire_dtype
        self.static_rows = static_rows
        self.deferred_ids = bool(deferred_ids)
        self.coalesce = bool(coalesce)
        if not dist.is_initialized():
            raise RuntimeError("ShardedModel needs torch.distributed to be initialised (one process per GPU)")
        if self.coalesce and not static_rows:
            raise NotImplementedError("coalesce=True is the static-shape step's option")
        if config.get("num_blocks", 1) != 1:
            raise NotImplementedError("num_blocks != 1 (see tlsan_amd.model.Model)")
        self.optimizer = config.get("optimizer", "sgd")
        if self.optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of %s" % (sorted(OPTIMIZERS),))
        if self.optimizer in LAZY_ADAGRAD_OPTIMIZERS:
            raise NotImplementedError("optimizer=%r: the owners' update is built for lazy_adam, lazy_rmsprop and lazy_adadelta; "
                                      "the Adagrad forms train on one GPU (tlsan_amd.model.Model)" % self.optimizer)
        # lazy_adam / lazy_rmsprop / lazy_adadelta: the owners apply the optimizer to the rows that arrived and to no other
        # (tlsan_shard_apply_lazy_opt) -- the lazy owner update's form, as the C ABI's lazy kinds need TLSAN_L2_LAZY
        self.lazy_opt = self.optimizer in LAZY_OPTIMIZERS
        if self.lazy_opt and not self.lazy:
            raise NotImplementedError("optimizer=%r: the lazy optimizers update only the rows that reach their owner, which is "
                                      "the lazy owner update: pass l2_mode='lazy'" % self.optimizer)
        if self.lazy_opt and static_rows:
            raise NotImplementedError("optimizer=%r: the static-shape step (static_rows, and with it graph capture and "
                                      "wire_dtype='bf16') is built for lazy-L2 SGD only: Adam's step count is a launch "
                                      "argument, and the static step's driver has no lazy optimizer" % self.optimizer)
        self.dropout = float(config.get("dropout", 0.0))
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self._seed = int(seed)
        if self.lazy and self.optimizer != "sgd" and not self.lazy_opt:
            raise NotImplementedError("l2_mode='lazy' is the SGD update's form; optimizer=%r sweeps every row" % self.optimizer)
        self.config = config
        self.lib = L.load()
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        U, I, Cc = config["user_count"], config["item_count"], config["cate_count"]
        self.U, self.I, self.C = U, I, Cc
        self.di, self.dc, self.Ls = config["itemid_embedding_size"], config["cateid_embedding_size"], config["Ls"]
        self.d, self.H = config["hidden_units"], config["num_heads"]
        # fused rows: items [item_emb | item_b | pad], users [user_emb | usert_emb | pad], one width
        self.W = max(self.di + 4, _ru4(self.di + self.Ls))
        self.router = KeyRouter(I, U, self.world, self.rank, group)
        self.cI, self.cU = self.router.cI, self.router.cU
        dev = self.device
        self.shard = torch.zeros(self.router.R, self.W, dtype=torch.float32, device=dev)
        self.cate_emb = torch.zeros(Cc, self.dc, dtype=torch.float32, device=dev)
        icl = np.asarray(item_cate_list, np.int32)
        # item -> category in key space (user / padding keys: -1 = in no category), so the compact
        # table's map is one gather
        ck = np.full(self.router.nkeys, -1, np.int32)
        ids = np.arange(I)
        ck[(ids % self.world) * self.router.R + ids // self.world] = icl
        self.cate_by_key = torch.as_tensor(ck).to(dev)
        dims_full = L.Dims(U, I, Cc, self.d, self.di, self.dc, self.H, self.Ls)
        self.dims_full = dims_full
        self.lay = L.DenseLayout()
        L.check(self.lib.tlsan_dense_layout_of(C.byref(dims_full), C.byref(self.lay)), "tlsan_dense_layout_of")
        self.dense = torch.zeros(self.lay.n_dense, dtype=torch.float32, device=dev)
        self.dense_KT = torch.zeros(self.d, self.d, dtype=torch.float32, device=dev)
        self.reg = float(config["regulation_rate"])
        self.clip = float(config["max_gradient_norm"])
        if self.W > 256 or self.world > 16:
            raise NotImplementedError("fused shard rows up to 256 floats, up to 16 ranks")
        self._sq = torch.zeros(2, dtype=torch.float64, device=dev)   # sums of squares: local shard rows, cate_emb
        self._fl = FlatLayout(self.lay.n_dense, Cc * self.dc, Cc if self.lazy_opt else 0)     # the all-reduced vector
        self._flat = torch.zeros(self._fl.size, dtype=torch.float32, device=dev)
        self._gn_local = torch.zeros(1, dtype=torch.float32, device=dev)
        self._step_dev = torch.zeros(4, dtype=torch.float32, device=dev)     # lr * coef, coef, (lazy:) lr * coef / P_new, P_new
        self.renorm_every = 4096
        self._P = torch.ones(1, dtype=torch.float32, device=dev)            # lazy L2: tables = P * stored
        if self.lazy:
            self._slots64 = torch.zeros(self.router.R * self.world, dtype=torch.int64, device=dev)
            self._lws = None
            self._sopt_lazy = L.ShardOptimizer(L.OPT_SGD, 0, 0.0, 0.0, 0.0, None, None, None, None, None, None,
                                               self._P.data_ptr())
        # adam / rmsprop / adadelta: accumulators laid out like what they belong to (RMSProp's first starts at one)
        self._sopt = None
        if self.optimizer != "sgd":
            kind, b1, b2, eps = OPTIMIZERS[self.optimizer]
            kind &= ~L.OPT_LAZY      # (the dense weights move under the dense kind; the lazy apply is a call of its own)
            one = 1.0 if self.optimizer in ("rmsprop", "lazy_rmsprop") else 0.0
            self.slots = dict(shard_s1=torch.full_like(self.shard, one), shard_s2=torch.zeros_like(self.shard),
                              cate_s1=torch.full_like(self.cate_emb, one), cate_s2=torch.zeros_like(self.cate_emb),
                              dense_s1=torch.full_like(self.dense, one), dense_s2=torch.zeros_like(self.dense))
            self._sopt = L.ShardOptimizer(kind, 0, b1, b2, eps, *[self.slots[k].data_ptr() for k in
                                          ("shard_s1", "shard_s2", "cate_s1", "cate_s2", "dense_s1", "dense_s2")])
        self.last_loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.last_gnorm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._ws = None
        self._flags = torch.zeros(self.router.nkeys, dtype=torch.int32, device=dev)   # zero at rest
        self._ews = None
        self._topk = TopKCounters()
        loc = np.arange(self.rank, I, self.world)
        self._icl_local = torch.as_tensor(np.concatenate([icl[loc], np.zeros(1, np.int32)])).to(dev)   # category of local item n
        self._slots_buf = torch.zeros(self.router.R * self.world, dtype=torch.int32, device=dev)  # zero at rest
        self._aws = torch.empty(int(self.lib.tlsan_shard_apply_workspace(self.router.R, Cc)), dtype=torch.uint8, device=dev)
        self._step = 0
        self._epoch = 0
        self.global_step = _Var(lambda: self._step)
        self.global_epoch_step = _Var(lambda: self._epoch)
        self.global_epoch_step_op = _Var(self._inc_epoch)
        self.train_writer = _Writer(os.path.join(config.get("model_dir", "."), "train"))
        self.eval_writer = _Writer(os.path.join(config.get("model_dir", "."), "eval"))
        self._dynamic = DynamicStep(self)       # also plans and fetches the forward-only batches of evaluation
        self._static = None                     # static_rows: a StaticStep, made at the first training batch
        if init == "device":
            # the same distributions drawn on the device, shard by shard (tables of 10^7 rows: the host draw of the whole
            # model on every rank takes minutes and tens of GB); NOT the values of Model(init="numpy") on one GPU
            self._init_on_device(config, seed)
        elif init == "numpy":
            self.set_params(Model.init_params(config, seed))   # identical on every rank (numpy, seeded)
        else:
            raise ValueError("init must be 'numpy' or 'device'")

    def _init_on_device(self, config, seed):
        di, Ls, cI = self.di, self.Ls, self.cI
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed) * 1000003 + self.rank)
        n_i = len(range(self.rank, self.I, self.world))
        n_u = len(range(self.rank, self.U, self.world))
        self.shard.zero_()
        li, lu = float(np.sqrt(6.0 / (self.I + di))), float(np.sqrt(6.0 / (self.U + di)))
        self.shard[:n_i, :di].uniform_(-li, li, generator=g)
        self.shard[cI:cI + n_u, :di].uniform_(-lu, lu, generator=g)
        self.shard[cI:cI + n_u, di:di + Ls] = -1.0
        small = dict(config, item_count=1, user_count=1)
        p = Model.init_params(small, seed)          # cate_emb and the dense weights: the host stream, the same on every rank
        self.cate_emb.copy_(torch.as_tensor(np.asarray(p["cate_emb"], np.float32)))
        self._P.fill_(1.0)
        self._load_dense_and_KT(p)
        self._refresh_squares()
        self._reset_step_state()

    # ------------------------------------------------------------------ helpers
    def pack_dense(self, p):
        return pack_dense(self.lay, self.d, self.H, p)

    def unpack_dense(self, flat):
        return unpack_dense(self.lay, self.d, self.H, flat)

    def _load_dense_and_KT(self, p):
        """The dense weights of p into `dense`, and dense_K's transpose into dense_KT."""
        d, lay = self.d, self.lay
        self.dense.copy_(torch.as_tensor(self.pack_dense(p)))
        self.dense_KT.copy_(self.dense[lay.K:lay.K + d * d].view(d, d).t())

    def _inc_epoch(self):
        self._epoch += 1
        return self._epoch

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def device_batch(self, batch, is_test=False):
        """Upload the batch and map its ids into the router's key space (elementwise, once)."""
        db = batch if isinstance(batch, DeviceBatch) else DeviceBatch(batch, self.device, is_test, self.Ls)
        if not hasattr(db, "keys"):
            r = self.router
            # Padded slots of the windows (zeros past sl / sl_new, input.py:41-51) must not put item 0 into the plan:
            # a row that only padding refers to receives no gradient, and the per-row gradient buffer of the step is
            # not zero-filled (every compact row is expected to be written by a use).  They take the key of the
            # sample's own candidate instead -- always a real use; the kernels weigh padded slots with exactly 0.
            cand = db.i.long()
            ar = torch.arange(self.Ls, device=db.i.device)[None, :]
            hist = torch.where(ar < db.sl.long()[:, None], db.hist_i.long(), cand[:, None])
            parts = [r.item_keys(cand), r.item_keys(hist.reshape(-1))]
            if db.Sn > 0:
                ar = torch.arange(db.Sn, device=db.i.device)[None, :]
                new = torch.where(ar < db.sl_new.long()[:, None], db.hist_i_new.reshape(db.B, db.Sn).long(), cand[:, None])
                parts.append(r.item_keys(new.reshape(-1)))
            if db.j is not None:
                parts.append(r.item_keys(db.j.long()))
            parts.append(r.user_keys(db.u.long()))
            db.keys = torch.cat(parts).to(torch.int32)
        return db

    # ------------------------------------------------------------------ training
    def dropout_seed(self, step=None):
        """As tlsan_amd.model.Model.dropout_seed: the same pattern on every rank (ranks differ by sample offset)."""
        step = self._step if step is None else step
        return ((self._seed * 0x9E3779B1) ^ ((step + 1) * 0x85EBCA77)) & 0xFFFFFFFF

    def train_async(self, batch, lr, next_batch=None, weight=1.0, sample0=0, after_next=None):
        """One step.  sample0: position of this rank's first sample in the global batch (dropout pattern).
          `weight`: this rank's share of the global mean when the ranks' batches differ in
        size, B_rank * world / B_global (1 when they are equal; 0 for a rank that only holds a
        placeholder row of a global batch smaller than the world).
          `next_batch` (optional): its routing plan is queued before this step's heavy
        kernels, so that the next step's host wait for the exchange sizes costs nothing.
          `after_next` (optional, static_rows): the batch after that; its plan is built two steps ahead, beside the
        second half of this step and all of the next, and is off the critical path altogether."""
        db = self.device_batch(batch)
        if not self.static_rows:
            return self._dynamic.train(db, lr, next_batch, weight, sample0)
        if self._static is None:
            self._static = StaticStep(self, db)
        return self._static.train(db, lr, next_batch, weight, sample0, after_next)

    def __del__(self):
        # plans still queued with the library's launch thread hold raw pointers into this model's buffers: let the
        # thread issue them before the buffers go (the streams then order their kernels before the frees)
        try:
            if getattr(self, "_static", None) is not None:
                self.lib.tlsan_shard_plans_flush()
        except Exception:
            pass

    def check_static_overflow(self):
        """Host check of the static exchange (synchronises): raises when a batch needed more row slots of one owner
        than the exchange holds -- the steps since then are wrong."""
        if self._static is not None:
            self._static.check_overflow()

    def capture_step(self, batch, next_batch, lr):
        """Record one static-shape step (this batch in the slot it is planned in, the next batch's plan on the side
        streams) in a HIP graph.  Replays must follow the order of capture: the step of `batch` expects its plan
        where the previous step left it.  Capture and replay alternately along a cycle whose length is a multiple of
        the number of plan slots (4):  g0 = capture(b0, b1); replay(g0); g1 = capture(b1, b2); replay(g1); ...;
        g3 = capture(b3, b0); replay(g3) -- then replay the graphs in that order.  lr is baked in."""
        if not self.static_rows:
            raise RuntimeError("capture_step needs static_rows (the exchange sizes of the dynamic step pass through the host)")
        db, ndb = self.device_batch(batch), self.device_batch(next_batch)
        if self._static is None or not self._static.warm:
            raise RuntimeError("capture_step: run one eager step first (one-time initialisation cannot be recorded)")
        return self._static.capture(db, ndb, lr)

    def replay(self, g):
        self._static.replay(g)

    def train(self, sess, batch, lr, add_summary=False):
        self.train_async(batch, lr)
        return float(self.last_loss.item())

    # ------------------------------------------------------------------ evaluation
    @contextlib.contextmanager
    def _eval_forward(self, batch, is_test=True, lj=False, ut=True):
        """The forward of a forward-only batch on its compact table (plan -> fetch -> compact views -> tlsan_forward):
        yields (db, (dims, cp, cb), li, lj, u_t) -- lj when asked and the batch has a j, u_t [B, d] when asked, None
        otherwise -- for the work the caller queues behind it, and waits for that work on the way out: the fetched
        table must stay alive until it has run."""
        db = self.device_batch(batch, is_test)
        if self._static is not None:   # static-shape training: plans announced ahead may be running on the side streams
            self._static.drain()       # (they use the same mark scratch as this plan)
        sl = self._dynamic.plan_eval(db)
        table = self._dynamic.fetch(sl)
        views = self._dynamic.compact(db, sl, table)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        li, lj, ut = new(db.B), new(db.B) if lj and db.j is not None else None, new(db.B, self.d) if ut else None
        ptr = lambda t: None if t is None else t.data_ptr()
        L.check(self.lib.tlsan_forward(*map(C.byref, views), li.data_ptr(), ptr(lj), ptr(ut), None, 0, self._stream()),
                "tlsan_forward")
        yield db, views, li, lj, ut
        torch.cuda.current_stream(self.device).synchronize()

    def forward(self, batch, is_test=True, want_ranks=False, exclude=None):
        with self._eval_forward(batch, is_test, lj=True, ut=want_ranks) as (db, views, li, lj, ut):
            ranks = self._ranks(db, *views, ut, exclude) if want_ranks else None
        return (li, lj, ranks) if want_ranks else (li, lj)

    def _gather_excl(self, off, xid, B):
        """The exclusion lists (exclusion_csr) of every rank's rows: slots of one width, padded to the widest rank's with
        ignored ids -> (off, ids) over the world * B all-gathered rows."""
        if off is None or self.world == 1:
            return off, xid
        w = int(off[1].item())
        width = int(allgather_rows(torch.tensor([w], device=self.device), self.group).max().item())
        rows = torch.full((B, width), np.iinfo(np.int32).max, dtype=torch.int32, device=self.device)
        rows[:, :w] = xid.view(B, w)
        xid = allgather_rows(rows, self.group).view(-1)
        off = torch.arange(0, (self.world * B + 1) * width, width, dtype=torch.int32, device=self.device)
        return off, xid

    def _ranks(self, db, dims, cp, cb, ut, exclude=None):
        """All-items ranking with the items sharded: the label's own score comes from the
        compact table of the rank that holds the user; u_t, label scores and label ids are
        all-gathered; every rank counts the items of ITS shard that rank ahead of each label
        (ties -> lower global id, tf.nn.top_k's order); one all-reduce of the counts gives the
        ranks.  Same kernels as the single-GPU tlsan_eval_ranks.
        exclude (Model.label_ranks' forms): the lists are all-gathered with u_t, every rank also counts the listed
        items of ITS shard (tlsan_eval_counts_shard_excl: those it holds, and those of them it counted ahead of the
        label), and the two counts ride in the same all-reduce -> (filtered ranks, eligible items) of this rank's rows."""
        B, st = db.B, self._stream()
        ws = grow_workspace(self, "_ws", self.lib.tlsan_workspace_bytes(C.byref(dims), B, 0), 1.25)
        s_lab = torch.empty(B, dtype=torch.float32, device=self.device)
        L.check(self.lib.tlsan_eval_label_scores(C.byref(dims), C.byref(cp), ut.data_ptr(), cb.i, B, s_lab.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), st), "tlsan_eval_label_scores")
        ut_all, s_all, lab_all = allgather_rows(ut, self.group), allgather_rows(s_lab, self.group), allgather_rows(db.i, self.group)
        Bt = int(ut_all.shape[0])
        nloc, ldims, lp = self._item_shard()
        ws = grow_workspace(self, "_ews", self.lib.tlsan_workspace_bytes(C.byref(ldims), Bt, 0), 1.25)
        head = (C.byref(ldims), C.byref(lp), ut_all.data_ptr(), s_all.data_ptr(), lab_all.data_ptr(), Bt, self.world, self.rank)
        tail = (ws.data_ptr(), ws.numel(), st)
        cah = torch.zeros(1 if exclude is None else 3, Bt, dtype=torch.int32, device=self.device)     # counts (, ahead, held)
        if exclude is None:
            if nloc > 0:
                L.check(self.lib.tlsan_eval_counts_shard(*head, cah[0].data_ptr(), *tail), "tlsan_eval_counts_shard")
        else:
            off, xid = self._gather_excl(*exclusion_csr(db, exclude, self.I), B)
            if nloc > 0:
                L.check(self.lib.tlsan_eval_counts_shard_excl(*head, off.data_ptr(), xid.data_ptr(), cah[0].data_ptr(),
                                                              cah[1].data_ptr(), cah[2].data_ptr(), *tail),
                        "tlsan_eval_counts_shard_excl")
        if self.world > 1:
            allreduce_sum(cah, self.group)
        mine = cah[:, self.rank * B:(self.rank + 1) * B]
        return mine[0] if exclude is None else (mine[0] - mine[1], (self.I - 1) - mine[2])

    def _item_shard(self):
        """This rank's items as a table of their own (local item n = global item n * world + rank): (local count,
        dims, params) for the all-items scoring."""
        nloc = ModPartition(self.I, self.world).local_count(self.rank)
        ldims = L.Dims(self.U, max(nloc, 1), self.C, self.d, self.di, self.dc, self.H, self.Ls)
        return nloc, ldims, fused_params(self, self.shard, self._icl_local)

    def _item_cate(self, g):
        """The categories of the global item ids g (an int64 device tensor), from the replicated map."""
        return self.cate_by_key[(g % self.world) * self.router.R + g // self.world]

    def item_scope(self, items=None, mask=None, categories=None):
        """Model.item_scope: an ItemScope over the model's items (every rank builds the same one)."""
        icl = None if categories is None else self._item_cate(torch.arange(self.I, device=self.device))
        return ItemScope(self.I, self.device, items=items, mask=mask, categories=categories, item_cate=icl)

    def item_boost(self, values=None, items=None, categories=None, base=0.0):
        """Model.item_boost: an ItemBoost over the model's items (every rank builds the same one, replicated)."""
        return item_boost_for(self.I, self.device, lambda: self._item_cate(torch.arange(self.I, device=self.device)), values, items,
                              categories, base)

    def last_item_categories(self, batch):
        """Model.last_item_categories for this rank's rows (no collective: the map is replicated)."""
        item = last_items(self.device_batch(batch, is_test=True))
        return torch.where(item >= 0, self._item_cate(item.clamp(min=0)), -1).to(torch.int32)

    def shortlist_index(self):
        """Model.shortlist_index is not built across ranks: per-shard certificates are a follow-up."""
        raise NotImplementedError("ShardedModel: a ShortlistIndex certifies a row against one table; per-shard certificates are not built")

    def shelves(self, *args, **kwargs):
        """Model.shelves is not built across ranks: a category's items are spread over the ranks."""
        raise NotImplementedError("ShardedModel: a category's items are spread over the ranks, so a rank cannot rank categories "
                                  "alone; the sharded form of shelves is not built")

    def cluster_index(self, *args, **kwargs):
        """Model.cluster_index is not built across ranks: a ValueError (train and probe a ClusteredIndex on a Model)."""
        raise ValueError("ShardedModel: a ClusteredIndex is not supported on a row-sharded model (building and probing across ranks)")

    def category_index(self, within=None):
        """Model.category_index: a CategoryIndex over the model's items or an ItemScope's (every rank builds the same one)."""
        return CategoryIndex(self._item_cate(torch.arange(self.I, device=self.device)), self.C, self.device,
                             within=scope_within(within, self.I))

    def recommend(self, batch, k, exclude=None, diversity=0.0, per_category=0, pool=None, within=None, category=None, index=None,
                  probes=None, boost=None, boost_weight=None, after=None):
        """Model.recommend for this rank's rows (every rank calls it, with the same k, exclusion mode and diversity
        settings): u_t and the exclusion lists are all-gathered, every rank selects the k best of ITS item shard for all
        rows (tlsan_eval_topk, global ids n * world + rank), each row's lists go to the rank that owns the row (one
        all-to-all) and are merged there (tlsan_topk_merge).  Same ids and scores as Model.recommend.
        diversity / per_category / pool (Model.recommend's second stage): the lists selected and merged are the pools
        of N entries; _rerank picks the k of each.  Same ids and score bits as Model.recommend on the gathered
        parameters.
        within / category (Model.recommend's; every rank passes the same scope, and its own rows' categories): each
        rank scans the scope's items ITS shard holds, within.sub(world, rank, its count), for all rows; the rows'
        categories are all-gathered with u_t.  The merge, the all-to-all and _rerank are unchanged.
        index (Model.recommend's; every rank passes the same index and the same P): each rank scans the lists of ITS
        item shard, index.local(world, rank, its count), for all gathered rows (tlsan_eval_topk_lists); the rows'
        category arrays are all-gathered with u_t, and the unrestricted rows among them run through the path without
        an index on every rank.
        boost / boost_weight (Model.recommend's; every rank passes the same boost, replicated and indexed by GLOBAL id,
        and its own rows' weights): the weights are all-gathered with u_t and every rank calls the boosted entry point
        (tlsan_eval_topk_scoped_boost / tlsan_eval_topk_lists_boost) with (id_mul, id_add) = (world, rank), so a column
        reads the boost of its global id.  The all-to-all, the merge and _rerank are unchanged: they see boosted scores.
        after (Model.recommend's; this rank's rows' ListCursor, every rank passes one or none does): the cursors are
        all-gathered with u_t and every rank calls the entry point behind a cursor (tlsan_eval_topk_scoped_after /
        tlsan_eval_topk_lists_after) on its shard with (world, rank): the cursor is in global ids, so every shard's list is
        behind the same position; the all-to-all and the merge are unchanged.  Same ids and score bits as
        Model.recommend(after=) on the gathered parameters."""
        after = None if after is None else cursor_of(after, batch_rows(batch), self.device)
        N = rerank_pool(k, diversity, per_category, pool)
        with self._recommend_lists(batch, after is not None, exclude, N, within, category, index, probes, boost, boost_weight) as topk:
            cid, csc = topk(int(k) if N is None else N, after)
            if N is not None:
                cid, csc = self._rerank(cid, csc, int(k), diversity, per_category)
        return cid, csc

    def recommend_deep(self, batch, n, page=256, **kw):
        """Model.recommend_deep for this rank's rows (collective: every rank calls it with the same n, page and forms):
        one forward, ceil(n / page) pages of ShardedModel.recommend(after=) chained on the device."""
        n, page = check_deep(n, page)
        after = kw.pop("after", None)
        after = None if after is None else cursor_of(after, batch_rows(batch), self.device)
        N = rerank_pool(page, kw.pop("diversity", 0.0), kw.pop("per_category", 0), kw.pop("pool", None))
        with self._recommend_lists(batch, True, kw.pop("exclude", None), N, kw.pop("within", None), kw.pop("category", None),
                                   kw.pop("index", None), kw.pop("probes", None), kw.pop("boost", None),
                                   kw.pop("boost_weight", None), **kw) as topk:
            return deep_pages(topk, n, page, after)

    @contextlib.contextmanager
    def _recommend_lists(self, batch, paged, exclude, N, within, category, index, probes, boost, boost_weight):
        """What recommend and recommend_deep share: recommend's argument checks (paged: the call takes a cursor, so the
        second stage is refused), one forward, the gathers of u_t, exclusion lists, categories and weights -> topk(n, after),
        valid inside the block: this rank's rows' merged lists of n entries behind the ListCursor `after` (None: the
        entry points without a cursor, as ever)."""
        refuse_clustered(index, probes)
        if isinstance(index, ShortlistIndex):
            raise NotImplementedError("ShardedModel: a ShortlistIndex certifies a row against one table; per-shard certificates are not built")
        if paged and N is not None:
            raise ValueError("after= beside diversity / per_category / pool: the greedy second stage is not a prefix order")
        boost = boost_of(boost, boost_weight, batch_rows(batch), self.I, self.device)
        within = scope_within(within, self.I)
        if recommend_index(index, within, self.I, self.C) is not None:
            category = index_categories(category, batch_rows(batch), self.C, self.device)
        else:
            category = scope_categories(category, batch_rows(batch), self.C, self.device)
        with self._eval_forward(batch) as (db, _, _, _, ut):
            B, st = db.B, self._stream()
            ut_all = allgather_rows(ut, self.group)
            Bt = int(ut_all.shape[0])
            off, xid = self._gather_excl(*exclusion_csr(db, exclude, self.I), B)
            nloc, ldims, lp = self._item_shard()
            tws = lambda nbytes: grow_workspace(self, "_tws", nbytes)
            if boost is not None and boost[1] is not None:
                boost = (boost[0], allgather_rows(boost[1], self.group))
            cat_all = None if category is None else allgather_rows(category, self.group)
            sub = None if within is None or nloc == 0 else within.sub(self.world, self.rank, nloc)
            found = {}      # (the unrestricted rows of an indexed call: read from the device once, by the first page)

            def topk(k, after):
                if after is not None:
                    after = ListCursor(allgather_rows(after.ids, self.group), allgather_rows(after.scores, self.group))
                if nloc > 0 and index is not None:
                    cid, csc = indexed_topk(self.lib, ldims, lp, ut_all, Bt, k, (off, xid), index, cat_all,
                                            self.world, self.rank, nloc, tws, st, boost=boost, after=after, found=found)
                elif nloc > 0 and (within is not None or category is not None or boost is not None or after is not None):
                    cid, csc = scoped_topk(self.lib, ldims, lp, ut_all, Bt, k, (off, xid), sub, cat_all, self.world, self.rank,
                                           tws, st, boost=boost, after=after)
                elif nloc > 0:
                    cid, csc = eval_topk(self.lib, ldims, lp, ut_all, Bt, k, (off, xid), self.world, self.rank, tws, st)
                else:
                    cid = torch.full((Bt, k), -1, dtype=torch.int32, device=self.device)
                    csc = torch.full((Bt, k), float("-inf"), dtype=torch.float32, device=self.device)
                if self.world > 1:
                    # rows [r B, (r + 1) B) belong to rank r: block s of what arrives is rank s's list of this rank's rows
                    rid, rsc = torch.empty_like(cid), torch.empty_like(csc)
                    a2a(rid, cid, None, None, self.group)
                    a2a(rsc, csc, None, None, self.group)
                    cid, csc = topk_merge(self.lib, rid.view(self.world, B, k).transpose(0, 1).contiguous(),
                                          rsc.view(self.world, B, k).transpose(0, 1).contiguous(), st)
                return cid, csc
            yield topk

    def _rerank(self, pid, psc, k, diversity, per_category):
        """The second stage of a diversified recommend on this rank's merged pools [B, N] (collective; B, N the same on
        every rank): the pool ids of a chunk of rows are all-gathered, every rank reads the stored vectors and inverse
        norms of the ids ITS item shard holds (tlsan_item_vectors, zeros for the others), one all-to-all returns each
        rank's rows and every entry's are SELECTED from the rank that holds its id, g % world (a sum would turn -0 into
        +0); the categories come from the replicated map; tlsan_rerank picks.  A chunk's all-gathered vectors stay
        within model.RERANK_STAGING bytes."""
        B, N = pid.shape
        st = self._stream()
        ids = torch.empty(B, k, dtype=torch.int32, device=self.device)
        scores = torch.empty(B, k, dtype=torch.float32, device=self.device)
        shard = self._item_shard()
        rows = rerank_chunk(N, self.d, self.world)
        for r0 in range(0, B, rows):
            vec, inv, cate, _ = self._fetch_entries(pid[r0:r0 + rows].reshape(-1), shard, st)
            rerank(self.lib, pid[r0:r0 + rows], psc[r0:r0 + rows], vec, inv, cate, k, diversity, per_category,
                   ids[r0:r0 + rows], scores[r0:r0 + rows], st)
        return ids, scores

    def _fetch_entries(self, flat, shard, st):
        """The staging of _rerank and list_metrics (collective; the same Q on every rank): for this rank's Q flattened
        global ids (-1: none) -> (vec [Q, d], inv [Q], cate [Q], g [Q] the ids clamped to 0, int64).  The ids are
        all-gathered, every rank reads the stored vectors and inverse norms of the ids ITS item shard holds
        (tlsan_item_vectors, zeros for the others), one all-to-all returns each rank's entries and every entry's are
        SELECTED from the rank that holds its id, g % world; the categories come from the replicated map."""
        W, d = self.world, self.d
        nloc, ldims, lp = shard
        Q = int(flat.shape[0])
        asked = allgather_rows(flat, self.group)           # rank r's entries at [r Q, (r + 1) Q)
        if nloc > 0:
            vec, inv = item_vectors(self.lib, ldims, lp, asked, W, self.rank, st)
        else:
            vec = torch.zeros(W * Q, d, dtype=torch.float32, device=self.device)
            inv = torch.zeros(W * Q, dtype=torch.float32, device=self.device)
        if W > 1:
            # block s of what arrives is rank s's reading of this rank's entries
            gvec, ginv = torch.empty_like(vec), torch.empty_like(inv)
            a2a(gvec, vec, None, None, self.group)
            a2a(ginv, inv, None, None, self.group)
            owner = torch.where(flat >= 0, flat % W, torch.zeros_like(flat)).long()
            vec = torch.gather(gvec.view(W, Q, d), 0, owner[None, :, None].expand(1, Q, d))[0].contiguous()
            inv = torch.gather(ginv.view(W, Q), 0, owner[None])[0].contiguous()
        g = flat.clamp(min=0).long()
        return vec, inv, self.cate_by_key[(g % W) * self.router.R + g // W], g      # (the replicated item -> category map)

    def list_metrics(self, ids, labels=None, item_weight=None, exposure=None):
        """Model.list_metrics for this rank's lists (collective: every rank calls it, with lists of the same shape
        [B, K]): the entries' vectors and inverse norms are fetched from the ranks that hold them exactly as the second
        stage of a diversified recommend fetches them (_fetch_entries), and tlsan_list_metrics reads no table, so the
        ListMetrics equal Model.list_metrics' on the gathered parameters bit for bit.  exposure counts this rank's
        lists only: the caller sums the ranks' counters."""
        ids, labels, item_weight = list_metric_inputs(ids, labels, item_weight, exposure, self.I, self.device)
        if self._static is not None:   # (plans announced ahead may be running on the side streams)
            self._static.drain()
        st, shard = self._stream(), self._item_shard()

        def measure(sub, lab):
            vec, inv, cate, g = self._fetch_entries(sub.reshape(-1), shard, st)
            return list_metrics(self.lib, sub, vec, inv, cate, lab, None if item_weight is None else item_weight[g],
                                exposure, st)
        return list_metrics_chunks(ids, labels, rerank_chunk(ids.shape[1], self.d, self.world), measure)

    def similar_items(self, items, k, metric="cosine", exclude=None, within=None, same_category=False, index=None, probes=None):
        """Model.similar_items, collective: every rank passes the same items (and k, metric, exclude, within, same_category) and every rank
        gets all Q lists.  Each rank reads the stored vectors and inverse norms of the queries ITS item shard holds
        (tlsan_item_vectors, zeros for the others); they are all-gathered and each query's are SELECTED from the one
        rank that holds it (a sum would turn -0 into +0); every rank selects the k nearest of its shard for all queries
        (tlsan_similar_topk, global ids n * world + rank), the lists are all-gathered and merged (tlsan_topk_merge).
        Same ids and score bits as Model.similar_items on the gathered parameters.  index (with same_category=True): every
        rank scans the lists of its own item shard, index.local(world, rank, its count) (tlsan_similar_topk_lists)."""
        refuse_clustered(index, probes)
        qids, mc, excl = similar_queries(items, self.I, metric, exclude, self.device)
        within = scope_within(within, self.I)
        index = similar_index(index, within, same_category, self.I, self.C)
        if self._static is not None:   # (plans announced ahead may be running on the side streams)
            self._static.drain()
        Q, k, st = int(qids.shape[0]), int(k), self._stream()
        nloc, ldims, lp = self._item_shard()
        if nloc > 0:
            vec, inv = item_vectors(self.lib, ldims, lp, qids, self.world, self.rank, st)
        else:
            vec = torch.zeros(Q, self.d, dtype=torch.float32, device=self.device)
            inv = torch.zeros(Q, dtype=torch.float32, device=self.device)
        if self.world > 1:
            owner = (qids % self.world).long()
            vec = torch.gather(allgather_rows(vec, self.group).view(self.world, Q, self.d), 0,
                               owner[None, :, None].expand(1, Q, self.d))[0].contiguous()
            inv = torch.gather(allgather_rows(inv, self.group).view(self.world, Q), 0, owner[None])[0].contiguous()
        tws = lambda nbytes: grow_workspace(self, "_tws", nbytes)
        if nloc > 0 and index is not None:
            cate = self._item_cate(qids.long()).to(torch.int32).reshape(-1, 1).contiguous()
            cid, csc = lists_similar_topk(self.lib, ldims, lp, vec, inv, qids, k, mc, excl,
                                          index.local(self.world, self.rank, nloc), cate, self.world, self.rank, tws, st)
        elif nloc > 0 and (within is not None or same_category):
            # (each rank scans the scope's items ITS shard holds; the queries' categories come from the replicated map)
            sub = None if within is None else within.sub(self.world, self.rank, nloc)
            cate = self._item_cate(qids.long()).to(torch.int32).contiguous() if same_category else None
            cid, csc = scoped_similar_topk(self.lib, ldims, lp, vec, inv, qids, k, mc, excl, sub, cate, self.world,
                                           self.rank, tws, st)
        elif nloc > 0:
            cid, csc = similar_topk(self.lib, ldims, lp, vec, inv, qids, k, mc, excl, self.world, self.rank, tws, st)
        else:
            cid = torch.full((Q, k), -1, dtype=torch.int32, device=self.device)
            csc = torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device)
        if self.world > 1:
            cid, csc = topk_merge(self.lib, allgather_rows(cid, self.group).view(self.world, Q, k).transpose(0, 1).contiguous(),
                                  allgather_rows(csc, self.group).view(self.world, Q, k).transpose(0, 1).contiguous(), st)
        return cid, csc

    def user_vectors(self, batches, real=None):
        """Model.user_vectors for this rank's rows, collective: every rank passes as many batches (a forward is an
        exchange; a rank without rows passes a placeholder batch with real 0, as the evaluation's shares do) -> this
        rank's UserVectors.  One all-gather of the row counts fixes row0 and n_total: the global rows are rank 0's rows,
        then rank 1's, and so on."""
        batches = batch_list(batches)
        real = kept_rows(real, len(batches))
        vec, user = [torch.empty(0, self.d, dtype=torch.float32, device=self.device)], [torch.empty(0, dtype=torch.int32, device=self.device)]
        for batch, n in zip(batches, real):
            with self._eval_forward(batch) as (db, _, _, _, ut):
                vec.append(ut[:n].clone())
                user.append(db.u[:n].to(torch.int32))
        vec, user = torch.cat(vec), torch.cat(user)
        counts = allgather_rows(torch.tensor([int(vec.shape[0])], device=self.device), self.group).tolist()
        return UserVectors(vec, user, self, self._step, row0=sum(counts[:self.rank]), n_total=sum(counts), group=self.group,
                           world=self.world)

    def audience(self, items, k, users, exclude=None, after=None):
        """Model.audience, collective: every rank passes the same items, k and exclusion (lists of GLOBAL row numbers,
        whole; or the same SeenItems) and its own UserVectors, and every rank gets all Q lists, in global row numbers
        (users.users_of maps them to user ids).  The queries' stored vectors are read on each item shard
        (tlsan_item_vectors, zeros for the others) and their item_b from the fused shard rows, both all-gathered and each
        query's SELECTED from the rank that owns it (never a sum: it would turn -0 into +0); each rank scans its own
        rows with id_add = row0 (a rank without rows contributes -1 / -inf lists); the ranks' lists are all-gathered and
        folded with tlsan_topk_merge.  Same rows and score bits as Model.audience on the gathered parameters and rows.
        after (Model.audience's; every rank passes the same cursors, in global row numbers): each rank scans its own rows
        behind them (tlsan_dense_topk_after, id_add = row0); the merge is unchanged."""
        topk, after = self._audience_lists(items, k, users, exclude, after)
        return topk(int(k), after)

    def audience_deep(self, items, n, users, page=256, exclude=None, after=None):
        """Model.audience_deep, collective (every rank passes the same items, n, page, exclusion and cursors): one read of
        the items' vectors, ceil(n / page) pages of ShardedModel.audience(after=) chained on the device."""
        n, page = check_deep(n, page)
        topk, after = self._audience_lists(items, page, users, exclude, after)
        return deep_pages(topk, n, page, after)

    def _audience_lists(self, items, k, users, exclude, after):
        """What audience and audience_deep share: the checks, the exclusion lists and the gather of the queries' vectors and
        biases -> (topk, the checked cursor): topk(k, after) every query's merged list of k rows behind the ListCursor
        `after` (None: tlsan_dense_topk, as ever)."""
        qids = audience_queries(items, k, self.I, self.device)
        after = cursor_of(after, int(qids.shape[0]), self.device)
        check_user_vectors(users, self, self._step, self.d, self.device)
        if users.n_total < 1:
            raise ValueError("users: no rows")
        excl = audience_exclusion(exclude, qids, users)
        if self._static is not None:   # (plans announced ahead may be running on the side streams)
            self._static.drain()
        Q, st, W = int(qids.shape[0]), self._stream(), self.world
        nloc, ldims, lp = self._item_shard()
        if nloc > 0:
            vec, _ = item_vectors(self.lib, ldims, lp, qids, W, self.rank, st)
        else:
            vec = torch.zeros(Q, self.d, dtype=torch.float32, device=self.device)
        mine = (qids % W) == self.rank
        local = torch.where(mine, torch.div(qids, W, rounding_mode="floor"), torch.zeros_like(qids)).long()
        bias = torch.where(mine, self.shard[local, self.di], torch.zeros(Q, dtype=torch.float32, device=self.device))
        if W > 1:
            owner = (qids % W).long()
            vec = torch.gather(allgather_rows(vec, self.group).view(W, Q, self.d), 0,
                               owner[None, :, None].expand(1, Q, self.d))[0].contiguous()
            bias = torch.gather(allgather_rows(bias, self.group).view(W, Q), 0, owner[None])[0]
        bias = bias.contiguous()
        scale = self._P.expand(Q).contiguous() if self.lazy else None

        def topk(k, after):
            if len(users) > 0:
                rid, rsc = dense_topk(self.lib, vec, users.vec, scale, bias, excl, users.row0, k,
                                      lambda nbytes: grow_workspace(self, "_tws", nbytes), st, after=after)
            else:
                rid = torch.full((Q, k), -1, dtype=torch.int32, device=self.device)
                rsc = torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device)
            if W > 1:
                rid, rsc = topk_merge(self.lib, allgather_rows(rid, self.group).view(W, Q, k).transpose(0, 1).contiguous(),
                                      allgather_rows(rsc, self.group).view(W, Q, k).transpose(0, 1).contiguous(), st)
            return rid, rsc
        return topk, after

    def _score_owned(self, ut, cand):
        """Scores of this rank's rows' candidates (u_t [B, d], cand [B, C] global ids; every rank calls it with the same
        C): u_t and the ids are all-gathered, every rank scores the ids of ITS item shard (global id n * world + rank)
        for all rows, one all-to-all returns each row's scores to its owner, which SELECTS each candidate's score from
        the rank that holds the id (a sum would turn -0 into +0).  Padding and ids outside the table score -inf."""
        B, Cn = cand.shape
        ut_all, cand_all = allgather_rows(ut, self.group), allgather_rows(cand, self.group)
        sc = torch.full((int(ut_all.shape[0]), Cn), float("-inf"), dtype=torch.float32, device=self.device)
        nloc, ldims, lp = self._item_shard()
        if nloc > 0:
            score_candidates(self.lib, ldims, lp, ut_all, cand_all, self.world, self.rank, self._stream(), scores=sc)
        if self.world == 1:
            return sc
        # rows [r B, (r + 1) B) belong to rank r: block s of what arrives is rank s's scores of this rank's rows
        got = torch.empty_like(sc)
        a2a(got, sc, None, None, self.group)
        owner = torch.where(cand >= 0, cand % self.world, torch.zeros_like(cand)).long()
        return torch.gather(got.view(self.world, B, Cn), 0, owner[None]).view(B, Cn)

    def score_candidates(self, batch, candidates):
        """Model.score_candidates for this rank's rows (every rank calls it, with the same C).  Same scores, bit for
        bit."""
        with self._eval_forward(batch) as (db, _, _, _, ut):
            return self._score_owned(ut, candidate_tensor(candidates, db.B, self.device))

    def sample_negatives(self, batch, n, seed=1234, row0=0, exclude="history"):
        """Model.sample_negatives for this rank's rows; row0 is the GLOBAL index of this rank's first row.  No
        collective: a row's negatives depend on (seed, row, label, exclusion, n) only."""
        db = self.device_batch(batch, is_test=True)
        return sample_negatives(self.lib, self.I, db.i, n, seed, row0, exclusion_csr(db, exclude, self.I), self._stream())

    def sampled_ranks(self, batch, n, seed=1234, row0=0, exclude="history"):
        """Model.sampled_ranks for this rank's rows (every rank calls it, with the same n); row0 is the GLOBAL index of
        this rank's first row.  Same ranks as Model.sampled_ranks."""
        with self._eval_forward(batch) as (db, _, _, _, ut):
            return sampled_ranks(self.lib, self.I, db, ut, n, seed, row0, exclude, self._score_owned, self._stream())

    def _hits(self, batch, n_valid=None):
        h = hits_and_rows(self.label_ranks(batch)[:n_valid])   # (rows past n_valid only pad this rank's share to the common size)
        if self.world > 1:                                      # hits and rows of the GLOBAL test batch
            h = allreduce_sum(torch.as_tensor(h, device=self.device), self.group).cpu().numpy()
        return h[:-1], int(h[-1])

    def eval_prec(self, sess, batch, n_valid=None):
        """Streaming precision_at_k over the global batch (model.py:265-281); cumulative like the reference's
        never-reset local variables (train.py:75-76,82).  Identical on every rank.  Every rank must pass
        the same number of rows (the all-gather is equal-sized); n_valid marks how many of them count."""
        return self._topk.add_prec(*self._hits(batch, n_valid))

    def eval_recall(self, sess, batch, n_valid=None):
        return self._topk.add_recall(*self._hits(batch, n_valid))

    def label_ranks(self, batch, exclude=None, return_eligible=False):
        """rank of the positive item among ALL items for each test row of this rank's batch (model.py:140-156).
        exclude / return_eligible: Model.label_ranks' -- the filtered rank among the items the row's list does not hold
        (the label is never excluded) and the number of items the label competes with; every rank calls it with the
        same exclusion mode.  Same integers as Model.label_ranks."""
        r = self.forward(batch, is_test=True, want_ranks=True, exclude=exclude)[2]
        if exclude is None:
            return (r, torch.full_like(r, self.I - 1)) if return_eligible else r
        return r if return_eligible else r[0]

    def pairs_ranked_right(self, batch):
        """Model.pairs_ranked_right for this rank's rows."""
        li, lj = self.forward(batch, is_test=True)
        return (li - lj) > 0

    def eval_auc(self, sess, batch):
        return float(self.pairs_ranked_right(batch).float().mean().item())

    # ------------------------------------------------------------------ inspection
    def _table_views(self):
        return self.shard[:self.cI], self.shard[self.cI:]

    def fold_scale(self):
        """lazy L2: multiply the scale into the stored tables (P -> 1); what is trained does not change.
        Done on a fixed schedule (renorm_every) so that P stays away from fp32 underflow, and before the
        parameters are read."""
        if not self.lazy or self.lazy_opt:     # (the lazy optimizers work on the stored values: P is 1 throughout)
            return
        P = self._P
        di, Ls = self.di, self.Ls
        self.shard[:self.cI, :di].mul_(P)
        self.shard[self.cI:, :di + Ls].mul_(P)
        self.cate_emb.mul_(P)
        self._P.fill_(1.0)
        self._refresh_squares()

    def _gather_tables(self, shard):
        """A fused [item | user] shard tensor of every rank -> full tables (numpy), on every rank."""
        if self.world > 1:
            # (RCCL gathers device buffers; gloo, used by the single-GPU multi-process tests, host ones)
            src = shard.cpu() if _staged(self.group) else shard
            outs = [torch.empty_like(src) for _ in range(self.world)]
            dist.all_gather(outs, src, group=self.group)
            outs = [o.cpu() for o in outs]
        else:
            outs = [shard.cpu()]
        I, U, G, di, Ls = self.I, self.U, self.world, self.di, self.Ls
        item = np.zeros((I, self.W), np.float32)
        user = np.zeros((U, self.W), np.float32)
        for r in range(G):
            t = outs[r].numpy()
            ni, nu = len(range(r, I, G)), len(range(r, U, G))
            item[r::G] = t[:ni]
            user[r::G] = t[self.cI:self.cI + nu]
        return dict(item_emb=item[:, :di].copy(), item_b=item[:, di].copy(),
                    user_emb=user[:, :di].copy(), usert_emb=user[:, di:di + Ls].copy())

    def gather_params(self):
        """Full (un-sharded) parameters on every rank, as numpy (tests / checkpoints)."""
        self.fold_scale()
        out = self._gather_tables(self.shard)
        out["cate_emb"] = self.cate_emb.cpu().numpy()
        out.update(self.unpack_dense(self.dense.cpu().numpy()))
        return out

    # ------------------------------------------------------------------ checkpoints (model.py:302-313)
    def save(self, sess=None, sharded=True):
        """Sharded checkpoint: every rank writes its own rows (TLSAN-<step>.shard<r>of<G>.npz: the fused
        [item | user] shard as it sits in HBM), rank 0 adds the replicated parts (cate_emb, dense weights,
        counters) and the config JSON -- nothing is gathered, so tables that exceed one host's memory
        can be saved.  sharded=False gathers everything to rank 0 and writes the single-GPU format of
        tlsan_amd.model.Model.save (restores into either model, any world size).  Returns the path prefix."""
        import json
        self.check_static_overflow()       # never write down the result of a truncated exchange
        self.fold_scale()
        os.makedirs(self.config["model_dir"], exist_ok=True)
        base = os.path.join(self.config["model_dir"], "TLSAN-%d" % self._step)
        if not sharded:
            full = self.gather_params()                      # (a collective: every rank takes part)
            slots = self.gather_slots()
            if self.rank == 0:
                write_checkpoint(base + ".npz", self._step, self._epoch, full, slots)
        else:
            sl = {} if self._sopt is None else {k: v.cpu().numpy() for k, v in self.slots.items()}
            np.savez("%s.shard%dof%d.npz" % (base, self.rank, self.world), shard=self.shard.cpu().numpy(),
                     cI=self.cI, W=self.W, item_count=self.I, user_count=self.U,
                     **{k: v for k, v in sl.items() if k.startswith("shard_")})
            if self.rank == 0:
                np.savez(base + ".replicated.npz", cate_emb=self.cate_emb.cpu().numpy(), dense=self.dense.cpu().numpy(),
                         global_step=self._step, global_epoch_step=self._epoch, world=self.world,
                         **{k: v for k, v in sl.items() if not k.startswith("shard_")})
        if self.rank == 0:
            json.dump(self.config, open(base + ".json", "w"), indent=2)
        if self.world > 1:
            dist.barrier(group=self.group)                   # the files exist when any rank returns
        return base

    def restore(self, sess, path):
        """`path`: the prefix save() returned (sharded checkpoint of the SAME world size), or a
        single-file .npz checkpoint of Model.save / save(sharded=False) -- then every rank keeps its rows."""
        if path.endswith(".npz"):
            step, epoch, params, slots = read_checkpoint(path, want_slots=self._sopt is not None)
            self.set_params(params)
            if slots is not None:                                        # the optimizer's accumulators (Model.save)
                self._set_slots(slots)
        else:
            rep_ = np.load(path + ".replicated.npz")
            if int(rep_["world"]) != self.world:
                raise ValueError("sharded checkpoint of %d ranks cannot be restored on %d (use sharded=False)"
                                 % (int(rep_["world"]), self.world))
            zs = np.load("%s.shard%dof%d.npz" % (path, self.rank, self.world))
            if tuple(zs["shard"].shape) != tuple(self.shard.shape) or int(zs["cI"]) != self.cI:
                raise ValueError("shard shape %s does not match this model" % (zs["shard"].shape,))
            self.shard.copy_(torch.as_tensor(zs["shard"]))
            self._P.fill_(1.0)
            self.cate_emb.copy_(torch.as_tensor(rep_["cate_emb"]))
            self.dense.copy_(torch.as_tensor(rep_["dense"]))
            K = self.dense[self.lay.K:self.lay.K + self.d * self.d].view(self.d, self.d)
            self.dense_KT.copy_(K.t())
            self._refresh_squares()
            if self._sopt is not None and "shard_s1" in zs.files:      # the optimizer's accumulators
                for k in self.slots:
                    self.slots[k].copy_(torch.as_tensor((zs if k.startswith("shard_") else rep_)[k]))
            step, epoch = int(rep_["global_step"]), int(rep_["global_epoch_step"])
        self._step, self._epoch = step, epoch
        self._reset_step_state()

    def _reset_step_state(self):
        """After the parameters or the step counter were replaced: forget everything that was keyed by the old
        step sequence (the stamped slots of the lazy owner update) or built for an announced successor."""
        if self.lazy:
            self._slots64.zero_()
        self._dynamic.reset()
        if self._static is not None:
            self._static.reset()

    def _shard_layout(self, p):
        """Full tables (dict of numpy arrays named like the parameters) -> this rank's fused [item | user] rows."""
        G, r, di, Ls = self.world, self.rank, self.di, self.Ls
        gi = np.arange(r, self.I, G)
        gu = np.arange(r, self.U, G)
        t = np.zeros(tuple(self.shard.shape), np.float32)
        t[:len(gi), :di] = np.asarray(p["item_emb"], np.float32)[gi]
        t[:len(gi), di] = np.asarray(p["item_b"], np.float32)[gi]
        t[self.cI:self.cI + len(gu), :di] = np.asarray(p["user_emb"], np.float32)[gu]
        t[self.cI:self.cI + len(gu), di:di + Ls] = np.asarray(p["usert_emb"], np.float32)[gu]
        return t

    def _set_slots(self, slots):
        """The two accumulator sets of adam / rmsprop / adadelta from full tables (Model.get_slots' format)."""
        for n, src in enumerate(slots, 1):
            self.slots["shard_s%d" % n].copy_(torch.as_tensor(self._shard_layout(src)))
            self.slots["cate_s%d" % n].copy_(torch.as_tensor(np.asarray(src["cate_emb"], np.float32)))
            self.slots["dense_s%d" % n].copy_(torch.as_tensor(self.pack_dense(src)))

    def gather_slots(self):
        """Full (un-sharded) optimizer accumulators on every rank, in Model.get_slots' format (None for sgd)."""
        if self._sopt is None:
            return None
        out = []
        for n in (1, 2):
            full = self._gather_tables(self.slots["shard_s%d" % n])
            full["cate_emb"] = self.slots["cate_s%d" % n].cpu().numpy()
            full.update(self.unpack_dense(self.slots["dense_s%d" % n].cpu().numpy()))
            out.append(full)
        return out

    def _refresh_squares(self):
        it, us = self._table_views()
        di, Ls = self.di, self.Ls
        # running sums of squares of the regularised tables (tf.nn.l2_loss terms, model.py:164-169)
        self._sq[0] = it[:, :di].double().pow(2).sum() + us[:, :di + Ls].double().pow(2).sum()
        self._sq[1] = self.cate_emb.double().pow(2).sum()
        self._flat[self._fl.table_sq] = self._sq[0].float()   # rides in the all-reduce

    def set_params(self, p):
        """Load full parameters (dict of numpy arrays); every rank keeps its own rows."""
        self.shard.copy_(torch.as_tensor(self._shard_layout(p)))
        self.cate_emb.copy_(torch.as_tensor(np.asarray(p["cate_emb"], np.float32)))
        self._P.fill_(1.0)
        self._load_dense_and_KT(p)
        self._refresh_squares()
        self._reset_step_state()

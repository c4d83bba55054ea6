"""The training step of the row-sharded model (tlsan_amd.dist.ShardedModel), in its two forms, and what they share.

One step on the main stream, in this order on every rank (four collectives, all on one communicator in program order):

  plan, stage 1 (tlsan_route_plan; normally queued one step AHEAD for the next batch): mark the
      rows the batch touches in an owner-major key space, compact the marks with one HIP scan
      (distinct rows already in all-to-all order + the id -> compact-row map), and tell every
      owner which of its rows are wanted with ONE equal-split all-to-all that carries counts and
      row numbers together; the counts are copied to pinned host memory behind an event;
  plan, stage 2: the host reads the counts (the only host wait of a step; free when stage 1 ran a
      step ahead);
  (1) owners gather the wanted rows (tlsan_shard_gather), all-to-all of the rows into a compact
      per-step table the HIP kernels run on in place (row strides, tlsan_params.ld_*);
  (2) fused forward/backward + exact per-row gradient sums written straight into the fused
      [rows, W] layout (tlsan_grads with strides / sparse rows);
  (3) ONE all-reduce of [dense grads | cate grads | loss | norm terms] (FlatLayout);
  (4) tlsan_shard_summary: global norm, clip coefficient, loss, dense update (one launch);
  (5) all-to-all of the per-row gradients back to the owners;
  (6) tlsan_shard_apply: the owners file each received row under (row, source rank) -- rows of one
      source are distinct, so no counting sort -- and apply the update with dense L2 decay to every
      local row in fixed source order (bitwise reproducible), category table included.  (l2_mode="lazy": only the rows
      that arrived -- tlsan_shard_apply_lazy for sgd, tlsan_shard_apply_lazy_opt for lazy_adam / lazy_rmsprop /
      lazy_adadelta, whose category-use flags ride in the all-reduce of (3).)

Items and users share one fused shard table and one exchange each way.

`DynamicStep` is that step with exchange sizes that follow the batch (they pass through the host once per step); it also
plans and fetches the forward-only batches of evaluation.  `StaticStep` (static_rows) exchanges a fixed number of row
slots per (source, owner) pair: no size reaches the host, the plans of announced batches are built on side streams (or
by the library's launch thread), and a step can be recorded in a HIP graph.  Both work on the buffers of the model they
are given (`m`), which owns the parameters.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import torch
import torch.distributed as dist

from . import _lib as L
from .dist_comm import _staged, a2a, allreduce_sum
from .model import _STARTED_WORDS, concurrent_streams, grow_workspace


_STATE_HDR_BYTES = 256   # sizeof(StateHdr), csrc/tlsan_state.h: what tlsan_state_reindex keeps
_STATIC_SLOTS = 4     # routing plans of the static-shape step: the current batch and up to two announced successors

# the announced batches' plans are issued by a launch thread of the library (tlsan_shard_step_static, TLSAN_PLAN_ASYNC);
# TLSAN_PLAN_THREAD=0 keeps them on the calling thread.  The thread has only ever run on one-GPU boxes, so it is the default
# at ONE rank only (where the step is bound by its host thread: 93.6 -> 83.9 us); over several ranks it is opt-in
# (TLSAN_PLAN_THREAD=1) until a node has exercised it -- there the exchanges, not the host, bound the step.
_PLAN_THREAD_ENV = os.environ.get("TLSAN_PLAN_THREAD")
_PLAN_THREAD = _PLAN_THREAD_ENV != "0"


# ---------------------------------------------------------------------- shared by the two forms
class FlatLayout:
    """The vector a step all-reduces, as offsets in floats:
      dense grads | cate grads | mean BCE | per-use squares | local table squares | pad
    and, for the lazy optimizers, | C category-use flags (1 where this rank's batch uses the category: the sum over the
    ranks is the number of ranks that use it, exact in fp32 and the same bits everywhere)."""
    __slots__ = ("n_dense", "n_cate", "cate", "loss", "use_sq", "table_sq", "cate_use", "size")

    def __init__(self, n_dense, n_cate, n_use_flags):
        self.n_dense, self.n_cate = n_dense, n_cate
        self.cate = n_dense
        self.loss = n_dense + n_cate
        self.use_sq, self.table_sq, self.cate_use = self.loss + 1, self.loss + 2, self.loss + 4
        self.size = self.cate_use + n_use_flags


def compact_batch(db, comp, Ls):
    """The batch with its ids replaced by rows of the compact table: the plan writes them into `comp` as
    i | hist | new | j | u."""
    B, Sn = db.B, db.Sn
    base, o = comp.data_ptr(), 0
    p_i = base + 4 * o; o += B
    p_hist = base + 4 * o; o += B * Ls
    p_new = base + 4 * o if Sn > 0 else db.hist_i_new.data_ptr(); o += B * Sn
    p_j = None
    if db.j is not None:
        p_j = base + 4 * o; o += B
    p_u = base + 4 * o
    ptr = lambda t: None if t is None else t.data_ptr()
    return L.Batch(B, Sn, p_u, p_i, p_j, ptr(db.y), p_hist, p_new, ptr(db.hist_t), ptr(db.sl), ptr(db.sl_new), ptr(db.u_cate))


def fused_params(m, table, item_cate):
    """Params over a table of fused fp32 rows ([emb | item_b or position weights | pad], items and users alike)."""
    base = table.data_ptr()
    return L.Params(base, base + 4 * m.di, base, base + 4 * m.di, m.cate_emb.data_ptr(), m.dense.data_ptr(),
                    m.dense_KT.data_ptr(), item_cate.data_ptr(), m.W, m.W, m.W, m.W, m._P.data_ptr() if m.lazy else None)


def fused_params_bf16(m, table, pitch, cate_bf16, item_cate):
    """... over wire rows: bf16 embedding values + fp32 tail in one slot of `pitch` bytes (strides in elements of each
    pointer's type), the category table through its bf16 shadow."""
    base = table.data_ptr()
    return L.Params(base, base + 2 * m.di, base, base + 2 * m.di, cate_bf16.data_ptr(), m.dense.data_ptr(),
                    m.dense_KT.data_ptr(), item_cate.data_ptr(), pitch // 2, pitch // 4, pitch // 2, pitch // 4,
                    m._P.data_ptr(), L.TABLE_BF16)


def step_outputs(m, gf):
    """(GradsOut, StepOut) of a step: per-row gradients land directly in the fused layout of `gf` (a compact row is an
    item or a user), everything else in the all-reduced vector."""
    fl, fp, g0, di, W = m._fl, m._flat.data_ptr(), gf.data_ptr(), m.di, m.W
    go = L.GradsOut(g0, g0 + 4 * di, g0, g0 + 4 * di, fp + 4 * fl.cate, fp, W, W, W, W, 2)
    return go, L.StepOut(fp + 4 * fl.loss, m._gn_local.data_ptr(), None, fp + 4 * fl.use_sq)


def scale_by_weight(m, gf, weight):
    """An uneven split of the global batch: the local means enter with their share (the per-use squares with its square)."""
    fl, flat = m._fl, m._flat
    flat[:fl.use_sq].mul_(float(weight))
    flat[fl.use_sq:fl.table_sq].mul_(float(weight) ** 2)
    gf.mul_(float(weight))


# ---------------------------------------------------------------------- the step whose exchange sizes pass through the host
class DynamicSlot:
    """Routing buffers and plan of one batch (DynamicStep keeps three: current / prefetched / forward-only)."""
    __slots__ = ("k", "cap", "pcap", "rank", "uniq", "n_uniq", "sendbuf", "recvbuf", "cate_c", "cate_pad", "comp", "host",
                 "event", "state", "dims_key", "db", "rb", "prepared", "prep_event", "stage2", "send", "recv", "n", "n_recv",
                 "recv_rows", "src_off", "compact")

    def __init__(self, k, cap, pcap, rows_pad, G, nkeys, dev):
        self.k, self.cap, self.pcap = k, cap, pcap
        self.rank = torch.empty(nkeys, dtype=torch.int32, device=dev)
        self.uniq = torch.empty(nkeys, dtype=torch.int32, device=dev)
        self.n_uniq = torch.zeros(1, dtype=torch.int32, device=dev)
        # per peer {count, local row numbers ...}: ONE equal-split all-to-all carries both
        self.sendbuf = torch.zeros(G, 1 + pcap, dtype=torch.int32, device=dev)
        self.recvbuf = torch.zeros(G, 1 + pcap, dtype=torch.int32, device=dev)
        self.cate_c = torch.empty(max(cap, rows_pad), dtype=torch.int32, device=dev)
        self.cate_pad = 0                 # category map entries [n_uniq, cate_pad) are set to -1 (stage 1)
        self.comp = torch.empty(cap, dtype=torch.int32, device=dev)
        self.host = torch.zeros(2, G, dtype=torch.int32).pin_memory()
        self.event = torch.cuda.Event()
        self.state, self.dims_key = None, None      # the kernels' state of the compact table, and the shape it is indexed for
        # stage 1: the batch planned into the slot, the buffer the owners read the wanted rows from
        self.db, self.rb = None, None
        self.prepared, self.prep_event = False, None    # the side stream has built (is building) this batch's indices
        # stage 2 (of the batch `stage2`): the exchange sizes as the host read them
        self.stage2 = None
        self.send = self.recv = self.recv_rows = self.src_off = None
        self.n = self.n_recv = 0
        self.compact = {}                 # cache of the ctypes views, see DynamicStep.compact


class DynamicStep:
    """The step with exchange sizes that follow the batch, and the plan / fetch / views of forward-only batches."""

    def __init__(self, m):
        self.m = m
        self.slots = [None, None, None]    # routing plans: current / prefetched / forward-only (evaluation)
        self.next_slot = 0
        self.rows_pad = 4096     # compact-table rows are padded (grow-only): the kernels' state layout is stable
        self.pcap = 65536        # shared per-owner capacity of the id exchange (see _slot)
        self.sizes = {}          # (compact rows, categories, B, Sn) -> (state bytes, workspace bytes)
        self.side, self.side_event = None, None
        self._keep = None        # the step's tensors, alive until the next step

    def reset(self):
        """Forget the plans (built for an announced successor of a step sequence that has been replaced)."""
        self.slots = [None, None, None]
        self.next_slot = 0

    # ------------------------------------------------------------------ routing plan (two stages)
    def _slot(self, k, n_keys):
        """Per-slot routing buffers (two slots: the plan of the next batch is built while the
        current one is in use)."""
        m, sl = self.m, self.slots[k]
        # rows one owner can be asked for by one rank: the id exchange is equal-split, so this capacity
        # must be the SAME on every rank -- it is a value all ranks share (self.pcap: a constant at first,
        # raised in lockstep by the overflow protocol of _plan_stage2), never this rank's batch size
        pcap = min(m.router.R, self.pcap)
        if sl is None or sl.cap < n_keys or sl.pcap != pcap:
            cap = max(int(n_keys * 1.25) + 16, sl.cap if sl is not None else 0)
            sl = self.slots[k] = DynamicSlot(k, cap, pcap, self.rows_pad, m.world, m.router.nkeys, m.device)
        return sl

    def _plan_stage1(self, db, k):
        """Device-only half: distinct rows grouped by owner, compact ids, and ONE all-to-all that
        tells every owner which of its rows are wanted (counts + row numbers); the copy of the
        counts to the host is queued, nothing waits."""
        m = self.m
        nk = int(db.keys.numel())
        sl = self._slot(k, nk)
        if sl.cate_c.numel() < self.rows_pad:    # the padded table grew since the slot was made
            sl.cate_c = torch.empty(self.rows_pad, dtype=torch.int32, device=m.device)
        sl.cate_pad = self.rows_pad               # category map entries [n_uniq, cate_pad) are set to -1
        r = m.router
        L.check(m.lib.tlsan_route_plan(db.keys.data_ptr(), nk, r.R, r.G, m.cate_by_key.data_ptr(),
                                       m._flags.data_ptr(), sl.rank.data_ptr(), sl.uniq.data_ptr(),
                                       sl.n_uniq.data_ptr(), sl.sendbuf.data_ptr(), sl.pcap,
                                       sl.cate_c.data_ptr(), sl.cate_pad, sl.comp.data_ptr(),
                                       sl.host.data_ptr(), m._stream()),     # send counts -> host[0]
                "tlsan_route_plan")
        if m.world > 1:
            a2a(sl.recvbuf.view(-1), sl.sendbuf.view(-1), None, None, m.group)
            rb = sl.recvbuf
        else:
            rb = sl.sendbuf
        sl.rb = rb
        if m.world > 1:      # what the peers ask of this rank (at one rank: the same numbers, see stage 2)
            sl.host[1].copy_(rb[:, 0], non_blocking=True)
        sl.event.record(torch.cuda.current_stream(m.device))
        sl.db = db
        sl.prepared = False
        return sl

    def _plan_stage2(self, sl):
        """Host half: read the exchange sizes (the step's only host wait; free when stage 1 was
        queued a step ahead)."""
        if sl.stage2 is sl.db:
            return sl
        m = self.m
        sl.event.synchronize()
        h = sl.host
        send = h[0].tolist()
        recv = h[1].tolist() if m.world > 1 else send
        over = [-x for x in send + recv if x < 0]
        if over:
            # some rank's batch may ask one owner for more rows than the shared capacity holds: it sent
            # -need in every header and no rows.  Every rank sees the same negative headers, so all of
            # them raise the capacity to the same value and repeat the plan (rare: the capacity only grows)
            self.pcap = int(max(over) * 1.25) + 16
            sl.stage2 = None
            return self._plan_stage2(self._plan_stage1(sl.db, sl.k))
        sl.n, sl.n_recv = int(sum(send)), int(sum(recv))
        sl.recv_rows = torch.empty(max(sl.n_recv, 1), dtype=torch.int32, device=m.device)
        off = [0]
        for c in recv:
            off.append(off[-1] + int(c))
        sl.send, sl.recv, sl.src_off, sl.stage2 = send, recv, (C.c_int32 * (m.world + 1))(*off), sl.db
        return sl

    def _plan(self, db):
        """The plan of a TRAINING batch: prefetched (train_async(..., next_batch=)) or built now."""
        k = self.next_slot
        sl = self.slots[k]
        if sl is None or sl.db is not db:
            if sl is not None and sl.prepared:
                raise RuntimeError("train_async: the batch announced as next_batch must be the next one trained "
                                   "(its destination index is already counted into the slot's state)")
            sl = self._plan_stage1(db, k)
        self.next_slot = 1 - k
        return self._plan_stage2(sl)

    def plan_eval(self, db):
        """The plan of a forward-only batch, in a slot of its own: evaluation may run between a training
        step and the successor it has announced (whose plan and indices are waiting in the other slots)."""
        return self._plan_stage2(self._plan_stage1(db, 2))

    def fetch(self, sl):
        """compact per-step table: row k = the owner's shard row of the k-th distinct key"""
        m = self.m
        if self.rows_pad < sl.n:        # compact-table rows, padded (grow-only) so the state layout is stable
            self.rows_pad = (sl.n + sl.n // 16 + 4095) // 4096 * 4096
        if sl.cate_pad < self.rows_pad:  # (rare) the table grew after this plan's category map was written
            cc = torch.full((self.rows_pad,), -1, dtype=torch.int32, device=m.device)
            cc[:sl.n] = sl.cate_c[:sl.n]
            sl.cate_c, sl.cate_pad = cc, self.rows_pad
        rows = torch.empty((max(sl.n_recv, self.rows_pad if m.world == 1 else 1), m.W), dtype=torch.float32, device=m.device)
        L.check(m.lib.tlsan_shard_gather(m.shard.data_ptr(), m.W, m.router.R, m.W, sl.rb.data_ptr(),
                                         sl.pcap, m.world, sl.n_recv, rows.data_ptr(),
                                         sl.recv_rows.data_ptr(), m._stream()), "tlsan_shard_gather")
        if m.world == 1:
            return rows
        table = torch.empty((self.rows_pad, m.W), dtype=torch.float32, device=m.device)
        a2a(table[:sl.n], rows[:sl.n_recv], sl.send, sl.recv, m.group)
        return table

    def compact(self, db, sl, table):
        """ctypes views (dims, params, batch) of the step on the compact table (cached per slot: building the three
        structs costs the host more than a kernel launch, and their pointers only change when a buffer does)"""
        key = (id(db), sl.comp.data_ptr(), sl.cate_c.data_ptr(), None if table is None else table.data_ptr(), self.rows_pad)
        hit = sl.compact.get(key)
        if hit is not None and hit[0] is db:
            return hit[1]
        if len(sl.compact) >= 8:
            sl.compact.clear()
        m = self.m
        cp = fused_params(m, m.shard if table is None else table, sl.cate_c)   # (None: only item_cate is looked at)
        # rows [n, pad) of the padded table are never referenced (no use, category -1)
        n = self.rows_pad
        out = L.Dims(n, n, m.C, m.d, m.di, m.dc, m.H, m.Ls), cp, compact_batch(db, sl.comp, m.Ls)
        sl.compact[key] = (db, out)
        return out

    def _prepare_side(self, ndb, nsl):
        """While the current step runs: on a second stream, rebuild the category index of the next
        step's compact table and build its destination index (both functions of the routing plan
        only).  Ordered by host waits on events that are already complete; no collective here."""
        m, st8 = self.m, nsl.state
        if st8 is None or nsl.n > self.rows_pad or nsl.dims_key != (self.rows_pad, m.C) or m._ws is None:
            return   # first use of the slot or the padded shape grows: the step does it inline
        dims, cp, cb = self.compact(ndb, nsl, None)
        if self.side is None:
            self.side = concurrent_streams(m.device, 1)[0]
            self.side_event = [torch.cuda.Event(), torch.cuda.Event()]
        sst = C.c_void_p(self.side.cuda_stream)
        L.check(m.lib.tlsan_state_recategorize(C.byref(dims), C.byref(cp), st8.data_ptr(), sst), "tlsan_state_recategorize")
        L.check(m.lib.tlsan_batch_index(C.byref(dims), C.byref(cb), cp.item_cate, st8.data_ptr(), 0, sst), "tlsan_batch_index")
        ev = self.side_event[self.next_slot]
        ev.record(self.side)
        nsl.prep_event = ev
        nsl.prepared = True

    def _buffers(self, sl, dims, cp, B, Sn, prepared=False):
        m = self.m
        skey = (dims.item_count, dims.cate_count, B, Sn)
        if skey not in self.sizes:
            nst = m.lib.tlsan_state_bytes(C.byref(dims))
            nws = m.lib.tlsan_workspace_bytes(C.byref(dims), B, Sn)
            if nst == 0 or nws == 0:
                raise L.TlsanError(m.lib.tlsan_last_error().decode())
            self.sizes[skey] = (nst, nws)
        nst, nws = self.sizes[skey]
        fresh = sl.state is None or sl.state.numel() < nst
        if fresh:
            sl.state = torch.zeros(int(nst * 1.5), dtype=torch.uint8, device=m.device)
            sl.state[:4].view(torch.float32).fill_(1.0)   # table scale P = 1 (the owners apply the decay)
        grow_workspace(m, "_ws", nws, 1.25)
        # the compact table's item -> category map changes every step: rebuild the category -> items
        # index for it; the use counters are zero between steps unless the (padded) shape changed
        key = (dims.item_count, dims.cate_count)
        if prepared and not fresh and sl.dims_key == key:
            return
        if fresh or sl.dims_key != key:
            sl.dims_key = key
            L.check(m.lib.tlsan_state_reindex(C.byref(dims), C.byref(cp), sl.state.data_ptr(), m._stream()),
                    "tlsan_state_reindex")
        else:
            L.check(m.lib.tlsan_state_recategorize(C.byref(dims), C.byref(cp), sl.state.data_ptr(), m._stream()),
                    "tlsan_state_recategorize")

    def _lazy_stamp(self):
        """Stamp of this step's entries in _slots64 (tlsan_shard_apply_lazy): 1 .. 2^32-2, never 0 (the value
        of a cleared slot); the slots are cleared whenever the sequence restarts."""
        m = self.m
        s = m._step % 0xFFFFFFFE
        if s == 0 and m._step > 0:
            m._slots64.zero_()
        return s + 1

    # ------------------------------------------------------------------ training
    def train(self, db, lr, next_batch, weight, sample0):
        m = self.m
        G = m.world
        sl = self._plan(db)
        ndb = None
        if next_batch is not None:
            ndb = m.device_batch(next_batch)
            self._plan_stage1(ndb, self.next_slot)
        prepared = sl.prepared and sl.n <= self.rows_pad
        sl.prepared = False
        if prepared:
            sl.prep_event.synchronize()      # the side stream finished this batch's indices
        table = self.fetch(sl)
        dims, cp, cb = self.compact(db, sl, table)
        self._buffers(sl, dims, cp, db.B, db.Sn, prepared)
        n, Cc, di, Ls, W = dims.item_count, m.C, m.di, m.Ls, m.W
        dev = m.device
        fl, flat = m._fl, m._flat
        fp = flat.data_ptr()
        g_cate, sumsq_f32, cate_use = fp + 4 * fl.cate, fp + 4 * fl.table_sq, fp + 4 * fl.cate_use
        # (every compact row below sl.n is used by this batch and written in full: no zero fill; the rows
        #  past it are padding that is never sent on)
        gf = torch.empty(n, W, dtype=torch.float32, device=dev)
        go, out = step_outputs(m, gf)
        hp = L.HParams(float(lr), 0.0, m.clip, L.NORM_TF18, L.L2_DENSE, 0, 1 if prepared else 0,   # reg: applied by the owners
                       m.dropout, m.dropout_seed() if m.dropout > 0.0 else 0, int(sample0))
        st = m._stream()
        L.check(m.lib.tlsan_grads(C.byref(dims), C.byref(cp), C.byref(cb), C.byref(hp), C.byref(go), C.byref(out),
                                  sl.state.data_ptr(), m._ws.data_ptr(), m._ws.numel(), st), "tlsan_grads")
        if weight != 1.0:
            scale_by_weight(m, gf, weight)
        if m.lazy_opt:
            # the categories this rank's batch uses: those of the items of its compact table (user rows: -1) and its u_cate
            L.check(m.lib.tlsan_shard_cate_use(sl.cate_c.data_ptr(), sl.n, db.u_cate.data_ptr(), db.B, Cc, cate_use, st),
                    "tlsan_shard_cate_use")
        # ---- one all-reduce: dense grads | cate grads | loss | per-use squares | local table squares
        if G > 1:
            allreduce_sum(flat, m.group)
        if m._sopt is not None:
            m._sopt.step = m._step + 1
        sopt = None if m._sopt is None else C.byref(m._sopt)
        if m.lazy and not m.lazy_opt:
            sopt = C.byref(m._sopt_lazy)
        L.check(m.lib.tlsan_shard_summary_opt(fp, fl.n_dense, fl.n_cate, G, float(lr), m.reg, m.clip,
                                              m._sq.data_ptr() + 8, m.dense.data_ptr(), m.dense_KT.data_ptr(),
                                              C.byref(m.dims_full), m._step_dev.data_ptr(),
                                              m.last_loss.data_ptr(), m.last_gnorm.data_ptr(), sopt, st),
                "tlsan_shard_summary")
        # ---- row gradients back to the owners, deterministic apply with dense L2 decay of every row
        if G > 1:
            vals = torch.empty((max(sl.n_recv, 1), W), dtype=torch.float32, device=dev)
            a2a(vals[:sl.n_recv], gf[:sl.n], sl.recv, sl.send, m.group)
        else:
            vals = gf
        # (the three owner updates start alike: the shard, the rows that arrived and where they go)
        rows = (m.shard.data_ptr(), W, m.cI, m.router.R, W, di, di + Ls, vals.data_ptr(), W, sl.recv_rows.data_ptr(), sl.n_recv,
                sl.src_off, G)
        if m.lazy_opt:
            lws = grow_workspace(m, "_lws", int(m.lib.tlsan_shard_apply_lazy_opt_workspace(sl.n_recv, Cc)), 1.5)
            L.check(m.lib.tlsan_shard_apply_lazy_opt(*rows, m._slots64.data_ptr(), self._lazy_stamp(),
                                                     1.0 / G, m._step_dev.data_ptr(), m.reg, m.cate_emb.data_ptr(),
                                                     Cc, m.dc, g_cate, cate_use, m._sq.data_ptr(), sumsq_f32,
                                                     sopt, float(lr), lws.data_ptr(), lws.numel(), st),
                    "tlsan_shard_apply_lazy_opt")
        elif m.lazy:
            lws = grow_workspace(m, "_lws", int(m.lib.tlsan_shard_apply_lazy_workspace(sl.n_recv, Cc)), 1.5)
            L.check(m.lib.tlsan_shard_apply_lazy(*rows, m._slots64.data_ptr(), self._lazy_stamp(),
                                                 1.0 / G, m._step_dev.data_ptr(), m.cate_emb.data_ptr(), Cc, m.dc,
                                                 g_cate, m._sq.data_ptr(), sumsq_f32, m._P.data_ptr(),
                                                 lws.data_ptr(), lws.numel(), st), "tlsan_shard_apply_lazy")
        else:
            L.check(m.lib.tlsan_shard_apply_opt(*rows, m._slots_buf.data_ptr(), 1.0 / G, m._step_dev.data_ptr(), m.reg,
                                                m.cate_emb.data_ptr(), Cc, m.dc, g_cate,
                                                m._sq.data_ptr(), sumsq_f32, sopt, float(lr),
                                                m._aws.data_ptr(), m._aws.numel(), st),
                    "tlsan_shard_apply")
        m._step += 1
        self._keep = (table, gf, vals, sl.recv_rows)
        if m.renorm_every and m._step % m.renorm_every == 0:
            m.fold_scale()          # (lazy L2; nothing to fold otherwise)
        if ndb is not None:
            nsl = self._plan_stage2(self.slots[self.next_slot])   # its counts arrived long ago
            self._prepare_side(ndb, nsl)
        return db


# ---------------------------------------------------------------------- the static-shape step (static_rows)
class StaticSlot:
    """Routing buffers, compact table and kernel state of one batch of the static-shape step, and where its plan stands:
      fresh     a plan of `db` sits in the slot and no step has consumed it (its destination index is counted into `state`);
      pending   ... and was built on the side streams, whose `done` events nobody has waited for yet;
      ids_sent  its id all-to-all has been issued (False: the step that uses the plan issues it, on the main stream)."""
    __slots__ = ("k", "rank", "uniq", "n_uniq", "sendbuf", "recvbuf", "cate_c", "comp", "rows", "table", "recv_rows", "state",
                 "done", "planned", "db", "fresh", "pending", "ids_sent", "views", "plan_args", "step_args")

    def __init__(self, k, G, nkeys, cap, kcap, pitch, state_bytes, dev):
        n = G * cap
        self.k = k
        self.rank = torch.empty(nkeys, dtype=torch.int32, device=dev)
        self.uniq = torch.empty(nkeys, dtype=torch.int32, device=dev)
        self.n_uniq = torch.zeros(1, dtype=torch.int32, device=dev)
        self.sendbuf = torch.zeros(G, 1 + cap, dtype=torch.int32, device=dev)
        self.recvbuf = torch.zeros(G, 1 + cap, dtype=torch.int32, device=dev) if G > 1 else None
        self.cate_c = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.comp = torch.zeros(kcap, dtype=torch.int32, device=dev)
        self.rows = torch.zeros(n, pitch, dtype=torch.uint8, device=dev)
        self.table = torch.zeros(n, pitch, dtype=torch.uint8, device=dev) if G > 1 else None
        self.recv_rows = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.state = torch.zeros(int(state_bytes), dtype=torch.uint8, device=dev)
        self.state[:4].view(torch.float32).fill_(1.0)     # table scale P = 1 (the owners apply the decay)
        self.done, self.planned = (torch.cuda.Event(), torch.cuda.Event()), torch.cuda.Event()
        for ev in self.done + (self.planned,):            # (a torch event gets its handle at its first record: the
            ev.record()                                   #  library's argument blocks hold the raw handles)
        self.db, self.fresh, self.pending, self.ids_sent = None, False, False, True
        self.views, self.plan_args, self.step_args = {}, {}, {}      # caches of ctypes blocks, keyed by batch identity

    def plan_into(self, db, pending, ids_sent):
        """A plan of `db` has been issued (or handed to the step's own call) into the slot."""
        self.db, self.fresh, self.pending, self.ids_sent = db, True, pending, ids_sent    # (a step consumes its plan: the destination index counts down to zero)

    def consume(self):
        """A step takes the slot's plan (whatever it had in flight has been waited for, or is on the step's stream)."""
        self.fresh = self.pending = False

    def discard(self):
        """The slot's plan will not be trained (and its index has been taken out of `state`)."""
        self.db, self.fresh, self.pending = None, False, False

    def announce_by_replay(self, db):
        """A replayed graph has built the plan of `db` here and joined its side streams."""
        self.db, self.fresh, self.pending = db, True, False

    def joined(self):
        """The side streams have been joined: nothing of the slot's plan is in flight."""
        self.pending = False

    def rewind(self, fresh):
        """A recording queued nothing: the slot's plan is (not) waiting, as before the step that was recorded."""
        self.fresh = fresh


class StaticStep:
    """The step with a fixed number of row slots per (source, owner) pair: its buffers, the plans of announced batches on
    two side streams, the library's launch thread, capture and replay.  Made at the model's first training batch."""
    __slots__ = ("m", "cap", "n", "kcap", "status", "status_host", "stamp", "gf", "vals", "lws", "slots", "next", "side", "side2",
                 "fork", "side_group", "checked", "warm", "started", "started_word", "start_seq", "prev_stamped", "dims", "wire",
                 "pitch", "tail", "cate_bf16")

    def __init__(self, m, db):
        """Buffers sized once, for batches like `db`: `cap` row slots per (source, owner) pair."""
        self.m = m
        r, G, dev, W = m.router, m.world, m.device, m.W
        self.next = 0                                   # the slot the next step's plan is (expected) in
        self.checked, self.warm = 0, False              # step of the last overflow check; one eager step has run
        self.start_seq, self.prev_stamped = 0, False    # number of the last stamped step; the step before carried a stamp
        self.side_group, self.cate_bf16 = None, None
        if m.static_rows is True:
            # what this batch needs of its busiest owner (one host read, at set-up only), with headroom; the
            # all-to-alls are equal-split, so every rank must use the same number
            flags = torch.zeros(r.nkeys, dtype=torch.int32, device=dev)
            flags[db.keys.long()] = 1
            need = int(flags.view(G, r.R).sum(1).max().item())
            t = torch.tensor([need], dtype=torch.int64, device=dev)
            if G > 1:
                if _staged(m.group):
                    c = t.cpu(); dist.all_reduce(c, op=dist.ReduceOp.MAX, group=m.group); t = c
                else:
                    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=m.group)
            cap = (int(t.item()) * 3 // 2 + 64 + 255) // 256 * 256
        else:
            cap = int(m.static_rows)
        self.cap = cap = max(1, min(cap, r.R))
        self.n = n = G * cap
        self.kcap = db.B * (m.Ls + L.SN_CAP + 3)      # ids of the largest batch the kernels take
        self.side, self.side2 = concurrent_streams(dev, 2)     # on hardware queues of their own (see there)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        # status_host: a pinned word the plan's kernel writes itself, and only on overflow (the count of the
        # overflowing owner); it is not a copy of `status`
        self.status_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.stamp = torch.ones(1, dtype=torch.int32, device=dev)           # uint32 on the device side; never 0
        self.gf = torch.zeros(n, W, dtype=torch.float32, device=dev)
        self.vals = torch.zeros(n, W, dtype=torch.float32, device=dev) if G > 1 else None
        self.lws = torch.empty(int(m.lib.tlsan_shard_apply_lazy_workspace(n, m.C)) + 256, dtype=torch.uint8, device=dev)
        self.fork = torch.cuda.Event()
        self.fork.record()
        self.started = torch.zeros(16, dtype=torch.int32).pin_memory()
        _STARTED_WORDS.append(self.started)          # (a queued step writes it when it starts: it outlives the model)
        self.started_word = C.c_uint32.from_address(self.started.data_ptr())
        if G > 1 and not m.deferred_ids and (_staged(m.group) or os.environ.get("TLSAN_SIDE_COMM", "0") == "1"):
            # the next batch's id exchange runs on the side stream while the main stream's collectives are in
            # flight: a communicator of its own keeps the two sequences independent.  Two RCCL communicators with
            # kernels in flight on one device are only safe if every rank's GPU schedules them in a compatible
            # order, which has never been exercised on hardware (the pool's boxes have one GPU): over RCCL this is
            # opt-in (TLSAN_SIDE_COMM=1); by default the id exchange of a plan built ahead is issued by the step that
            # uses it, on the main stream (one more small all-to-all on the critical path, no second communicator).
            # The host-staged gloo exchange of the tests is serial either way and keeps the side group.
            ranks = list(range(G)) if m.group is None else dist.get_process_group_ranks(m.group)
            self.side_group = dist.new_group(ranks, backend=dist.get_backend(m.group))
            # communicators are set up at their first collective: do that here, on every rank at the same point, not in
            # the middle of the first step with the main communicator's collectives in flight
            warm = torch.zeros(G, dtype=torch.int32, device=dev)
            a2a(torch.empty_like(warm), warm, None, None, self.side_group)
            torch.cuda.synchronize(dev)
        self.dims = dims = L.Dims(n, n, m.C, m.d, m.di, m.dc, m.H, m.Ls)
        nst = m.lib.tlsan_state_bytes(C.byref(dims))
        nws = m.lib.tlsan_workspace_bytes(C.byref(dims), db.B, L.SN_CAP)
        if nst == 0 or nws == 0:
            raise L.TlsanError(m.lib.tlsan_last_error().decode())
        grow_workspace(m, "_ws", nws)
        self.wire = m.wire_dtype == "bf16"
        self.tail = max(1, m.Ls)                              # fp32 floats after the embedding: item_b / the position weights
        self.pitch = (2 * m.di + 4 * self.tail + 15) // 16 * 16 if self.wire else 4 * W      # bytes per slot of the compact table
        if self.wire:
            if m.di % 4:
                raise NotImplementedError("wire_dtype='bf16': embedding widths must be multiples of 4")
            self.cate_bf16 = torch.zeros(m.C, m.dc, dtype=torch.bfloat16, device=dev)
        self.slots = [StaticSlot(k, G, r.nkeys, cap, self.kcap, self.pitch, nst, dev) for k in range(_STATIC_SLOTS)]

    def _views(self, sl, db):
        """ctypes views of a batch on a slot's compact table (cached: the pointers are constants of the pair)"""
        hit = sl.views.get(id(db))
        if hit is not None and hit[0] is db:
            return hit[1]
        if len(sl.views) >= 16:
            sl.views.clear()
        m = self.m
        if int(db.keys.numel()) > self.kcap:
            raise ValueError("static_rows: this batch holds more ids than the buffers were sized for (batch size grew?)")
        table = sl.rows if m.world == 1 else sl.table
        if self.wire:
            cp = fused_params_bf16(m, table, self.pitch, self.cate_bf16, sl.cate_c)
        else:
            cp = fused_params(m, table, sl.cate_c)
        out = (cp, compact_batch(db, sl.comp, m.Ls))
        sl.views[id(db)] = (db, out)
        return out

    def _step_args(self, sl, db):
        """tlsan_static_step of (slot, batch): every pointer of the step's four launches (cached; lr, the dropout seed and
        the sample offset are filled in per step)."""
        m = self.m
        hit = sl.step_args.get(id(db))
        if hit is not None and hit[0] is db and hit[2] is m._ws:     # (the workspace may have been re-allocated)
            return hit[1]
        if len(sl.step_args) >= 16:
            sl.step_args.clear()
        G, W, di, Ls, Cc = m.world, m.W, m.di, m.Ls, m.C
        cp, cb = self._views(sl, db)
        fl, gf = m._fl, self.gf
        fp = m._flat.data_ptr()
        rb = (sl.recvbuf if G > 1 else sl.sendbuf).data_ptr()
        ss = L.StaticStep()
        ss.shard, ss.ld, ss.R, ss.W, ss.recvbuf, ss.cap, ss.G = m.shard.data_ptr(), W, m.router.R, W, rb, self.cap, G
        ss.rows_out, ss.recv_rows = sl.rows.data_ptr(), sl.recv_rows.data_ptr()
        ss.slots64, ss.stamp = m._slots64.data_ptr(), self.stamp.data_ptr()
        ss.wire, ss.d_emb, ss.tail, ss.pitch = (1 if self.wire else 0), di, self.tail, self.pitch
        ss.dims, ss.cp, ss.cb = C.pointer(self.dims), C.pointer(cp), C.pointer(cb)
        ss.hp = L.HParams(1.0, 0.0, m.clip, L.NORM_TF18, L.L2_DENSE, 0, 1, m.dropout, 0, 0)
        ss.go, ss.out = step_outputs(m, gf)
        ss.state, ss.ws, ss.ws_bytes = sl.state.data_ptr(), m._ws.data_ptr(), m._ws.numel()
        ss.flat, ss.n_dense, ss.n_cate, ss.lr, ss.reg, ss.clip = fp, fl.n_dense, fl.n_cate, 1.0, m.reg, m.clip
        ss.S_cate, ss.dense, ss.dense_KT = m._sq.data_ptr() + 8, m.dense.data_ptr(), m.dense_KT.data_ptr()
        ss.dims_full, ss.step_dev = C.pointer(m.dims_full), m._step_dev.data_ptr()
        ss.loss_out, ss.gnorm_out, ss.opt = m.last_loss.data_ptr(), m.last_gnorm.data_ptr(), C.pointer(m._sopt_lazy)
        ss.cI, ss.reg_item, ss.reg_user = m.cI, di, di + Ls
        ss.vals, ss.ldv, ss.marked, ss.gscale = (self.vals if G > 1 else gf).data_ptr(), W, 1, 1.0 / G
        ss.cate_emb, ss.C, ss.dc, ss.g_cate = m.cate_emb.data_ptr(), Cc, m.dc, fp + 4 * fl.cate
        ss.sumsq_out, ss.sumsq_f32, ss.scale = m._sq.data_ptr(), fp + 4 * fl.table_sq, m._P.data_ptr()
        ss.lws, ss.lws_bytes = self.lws.data_ptr(), self.lws.numel()
        sl.step_args[id(db)] = (db, ss, m._ws)
        return ss

    def flush(self):
        """Plans handed to the library's launch thread (tlsan_shard_step_static, TLSAN_PLAN_ASYNC) are issued when that
        thread gets to them: wait until it has, before anything on this thread that must come BEHIND a plan's launches
        (waiting on its events or streams, clearing what it writes, a stream capture)."""
        L.check(self.m.lib.tlsan_shard_plans_flush(), "tlsan_shard_plans_flush")

    def drain(self):
        """The main stream behind everything the announced plans have in flight (they share their mark scratch, and their
        slots' buffers, with whatever comes next): the launch thread has issued them, both side streams are joined."""
        main = torch.cuda.current_stream(self.m.device)
        self.flush()
        main.wait_stream(self.side)
        main.wait_stream(self.side2)
        return main

    def reset(self):
        """After the parameters or the step counter were replaced: no plan is pending, the stamps restart."""
        self.stamp.fill_(1)
        self.next = 0
        main = self.drain()
        for sl in self.slots:
            if sl.fresh:            # a plan nobody will train: its counters must not meet the next plan's
                self._discard(sl, main)
            sl.discard()

    def _discard(self, sl, stream):
        """A plan that was built into the slot and never trained (an announcement that was abandoned, a restore, a
        capture over a slot an eager step had planned): its destination index is still counted into the slot's
        state -- tlsan_batch_index only ADDS to the use counters, the step that consumes a plan counts them back to
        zero -- so a second plan on top would double every count and the row sums would run past their segments.
        Clear everything behind the state's header (the category index is rebuilt by every plan anyway), after
        whatever the abandoned plan still has in flight."""
        if not torch.cuda.is_current_stream_capturing():
            self.flush()
        if sl.pending and not torch.cuda.is_current_stream_capturing():
            stream.wait_event(sl.done[0])
            stream.wait_event(sl.done[1])
        with torch.cuda.stream(stream):
            sl.state[_STATE_HDR_BYTES:].zero_()
        sl.discard()

    def _plan_args(self, sl, db, stream, group, stream2):
        """tlsan_static_plan of (slot, batch, streams): the pointers are constants of the combination (cached)."""
        m = self.m
        r = m.router
        key = (id(db), stream.cuda_stream, None if stream2 is None else stream2.cuda_stream)
        hit = sl.plan_args.get(key)
        if hit is not None and hit[0] is db:
            return hit[1]
        if len(sl.plan_args) >= 16:
            sl.plan_args.clear()
        cp, cb = self._views(sl, db)
        ids_here = self._ids_in_plan(stream, group)
        pa = L.StaticPlan(db.keys.data_ptr(), int(db.keys.numel()), r.R, r.G, m.cate_by_key.data_ptr(),
                          m._flags.data_ptr(), sl.rank.data_ptr(), sl.uniq.data_ptr(), sl.n_uniq.data_ptr(),
                          sl.sendbuf.data_ptr(), self.cap, sl.cate_c.data_ptr(), sl.comp.data_ptr(),
                          self.status.data_ptr(), self.status_host.data_ptr(),
                          C.pointer(self.dims), C.pointer(cp), C.pointer(cb), sl.state.data_ptr(),
                          stream.cuda_stream, None if stream2 is None else stream2.cuda_stream,
                          None, sl.planned.cuda_event, sl.done[0].cuda_event if stream2 is not None else None,
                          sl.done[1].cuda_event if stream2 is not None else None,
                          1 if (stream2 is not None and not ids_here) else 0)
        sl.plan_args[key] = (db, pa)
        return pa

    def _ids_in_plan(self, stream, group):
        """Does the plan carry its own id all-to-all (on `stream`)?  Over several ranks: yes when it is built in line on
        the main stream, or ahead on a side stream with a communicator of its own (or over the host-staged gloo exchange
        of the tests, which is serial anyway); a plan built ahead WITHOUT one (the default over RCCL, see __init__;
        deferred_ids=True forces it anywhere) leaves the exchange to the step that uses it, in the main communicator's
        program order."""
        m = self.m
        if m.world == 1:
            return False
        if stream == torch.cuda.current_stream(m.device):
            return True
        if m.deferred_ids:
            return False
        return group is not None or _staged(m.group)

    def _plan(self, db, k, stream, group, stream2=None, defer=False):
        """Routing plan of `db` into slot k, destination index included: device work only, queued on `stream`
        (the destination index on `stream2` when given: it needs the plan's compact ids, the category index needs its
        category map -- two independent tails; the slot's `done` events then mark their ends).  One library call
        (tlsan_shard_plan_static); defer=True returns its argument block instead of issuing it (the step's own call
        issues it behind its forward/backward kernel) -- only for plans whose id exchange is not part of the plan."""
        m, sl = self.m, self.slots[k]
        if sl.fresh:          # an unconsumed plan sits in the slot: take its index out first
            self._discard(sl, stream)
        pa = self._plan_args(sl, db, stream, group, stream2)
        # (the overflow word travels to pinned host memory behind the plan that may have raised it, on the plan's own
        #  stream; the next steps look at the copy without synchronising.  Not part of a recording.)
        pa.status_host = None if torch.cuda.is_current_stream_capturing() else self.status_host.data_ptr()
        ids_here = not defer and self._ids_in_plan(stream, group)
        if not defer:
            L.check(m.lib.tlsan_shard_plan_static(C.byref(pa)), "tlsan_shard_plan_static")
            # what follows the plan's launches on the host: the id exchange, when the plan carries it, and the event behind it
            if ids_here:
                with torch.cuda.stream(stream):
                    a2a(sl.recvbuf.view(-1), sl.sendbuf.view(-1), None, None, group if group is not None else m.group)
                if stream2 is not None:
                    sl.done[0].record(stream)
        sl.plan_into(db, stream2 is not None, m.world == 1 or ids_here)
        return pa if defer else None

    def check_overflow(self):
        """Host check of the static exchange (synchronises): raises when a batch needed more row slots of one owner
        than the exchange holds -- the steps since then are wrong."""
        self.flush()
        need = int(self.status.item())
        if need > self.cap:
            raise RuntimeError("static_rows: a batch needed %d rows of one owner, the exchange holds %d per pair; "
                               "rebuild the model with static_rows >= %d" % (need, self.cap, need))

    def train(self, db, lr, next_batch, weight, sample0, after_next=None):
        m = self.m
        G = m.world
        NS = _STATIC_SLOTS
        main = torch.cuda.current_stream(m.device)
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            # an exchange that overflowed (a plan needed more rows of one owner than `cap`) truncates the step on the
            # device: seen here one or two steps later through the pinned copy -- not at the next 1024-step check
            need = int(self.status_host[0])
            if need > self.cap:
                raise RuntimeError("static_rows: a batch planned around step %d needed %d rows of one owner, the exchange "
                                   "holds %d per pair: the steps since then are wrong; rebuild the model with static_rows >= %d"
                                   % (m._step, need, self.cap, need))
        k = self.next
        slots = self.slots
        sl = slots[k]
        planned_inline = False
        if sl.db is not db or not sl.fresh:      # not announced by an earlier step: plan it now, in line
            planned_inline = True
            if not capturing:
                self.drain()     # (whatever an abandoned announcement left running in the slots)
            self._plan(db, k, main, m.group)
        elif sl.pending:
            if not capturing:                    # (recorded steps join their side work at their own end)
                # a HOST wait: announced two batches ahead the plan is long done, and a device-side wait is a barrier packet
                # in the main queue (~6 us of idle GPU each; the single-GPU Model waits on the host for the same reason)
                self.flush()                         # (the launch thread has recorded the events by then)
                sl.done[0].synchronize()
                sl.done[1].synchronize()
        sl.consume()
        if G > 1 and not sl.ids_sent:     # (plan built ahead without a side communicator: see _plan)
            a2a(sl.recvbuf.view(-1), sl.sendbuf.view(-1), None, None, m.group)
            sl.ids_sent = True
        self.next = (k + 1) % NS
        ahead = [(m.device_batch(b), (k + 1 + j) % NS) for j, b in enumerate((next_batch, after_next)) if b is not None]
        ahead = [(b, kk) for b, kk in ahead if not (slots[kk].db is b and slots[kk].fresh)]
        # EVERY eager step stamps the pinned word when its fused kernel starts (not only the steps that announce a batch:
        # a plan waits for "step t - 1 has started", which only names step t - 1 if that step carried a stamp -- ADVICE r4).
        # The word paces a plan only when the step before this one was such a stamped eager step; behind a graph replay, a
        # capture or the first step of a model the plans are ordered by an event on the main stream instead.
        stamp = not capturing
        # (... nor when this step has just planned its own batch in line, on the main stream: the plans share their mark
        #  scratch, and "the step before has started" says nothing about a plan queued behind it -- the event does)
        use_flag = bool(ahead) and stamp and self.prev_stamped and not planned_inline     # (see tlsan_shard_step_static: no event on the main stream)
        if ahead and not use_flag:
            self.fork.record(main)      # everything before this step: the slots the new plans go to are free from here

        # The step is issued in as few library calls as there are collectives in it (tlsan_shard_step_static: one at one
        # rank) from an argument block that is a constant of (slot, batch) -- as ~15 Python-level calls the HOST took
        # 100 us per step for 77 us of kernels.  Where the plans of the announced batches go in the launch order (the
        # device-side dependencies are the same either way): behind the forward/backward.  That kernel fills the GPU,
        # so a plan can only run beside the small kernels around it; queued ahead of it, the plan delays it (one rank,
        # same box: graph replay 113 us with the plan queued after the kernel, 153 us before).
        ss = self._step_args(sl, db)
        ss.hp.lr = float(lr); ss.lr = float(lr)
        ss.hp.dropout_seed = m.dropout_seed() if m.dropout > 0.0 else 0
        ss.hp.dropout_sample0 = int(sample0)
        sp = C.c_void_p(main.cuda_stream)
        flat, gf = m._flat, self.gf
        side, side2, side_group = self.side, self.side2, self.side_group
        plans, late = [], []          # argument blocks the step's own call issues / plans whose id exchange Python issues
        for b_, kk in ahead:
            if self._ids_in_plan(side, side_group):
                late.append((b_, kk))
            else:
                pa = self._plan(b_, kk, side, side_group, side2, defer=True)
                pa.ev_fork = None if use_flag else self.fork.cuda_event
                plans.append(pa)
        parr = (C.POINTER(L.StaticPlan) * max(1, len(plans)))(*[C.pointer(x) for x in plans]) if plans else None

        def run(phases, with_plans=False):
            # (plans: issued by the library's launch thread while this one goes on with the main stream -- not under capture)
            if with_plans and plans and use_flag and _PLAN_THREAD and (G == 1 or _PLAN_THREAD_ENV == "1"):
                phases |= L.PLAN_ASYNC
            L.check(m.lib.tlsan_shard_step_static(C.byref(ss), phases, parr if with_plans else None,
                                                  len(plans) if with_plans else 0, sp), "tlsan_shard_step_static")

        if stamp:         # the fused kernel stores the step's number into a pinned word when it begins to run
            self.start_seq = seq = (self.start_seq + 1) & 0xFFFFFFFF       # (the full 32 bits: the library compares (int32)(word - after))
            ss.out.started, ss.out.started_value = self.started.data_ptr(), seq
            # the announced batches' plans go to slots that steps t - 2 and t - 3 were the last to use: "step t - 1 has
            # started" is all they wait for -- long true when this step is queued, so the host does not block
            ss.plans_after = (seq - 1) & 0xFFFFFFFF
        else:
            ss.out.started, ss.out.started_value = None, 0

        def plan_late():
            if use_flag:
                word, want, t0, polls = self.started_word, (self.start_seq - 1) & 0xFFFFFFFF, None, 0
                while ((word.value - want) & 0xFFFFFFFF) >= 0x80000000:     # (not yet reached: the library's (int32)(word - after) < 0)
                    polls += 1
                    if polls & 255:
                        continue
                    time.sleep(0)
                    if t0 is None:
                        t0 = time.perf_counter()
                    elif time.perf_counter() - t0 > 30.0:
                        raise RuntimeError("train_async: the step's first kernel did not start within 30 s")
            else:
                side.wait_event(self.fork)
            for b_, kk in late:
                self._plan(b_, kk, side, side_group, side2)

        if self.wire:
            self.cate_bf16.copy_(m.cate_emb)      # (round to nearest even; the table is small and replicated)
        if G == 1 and weight == 1.0 and not late:
            run(L.PHASE_GATHER | L.PHASE_GRADS | L.PHASE_SUMMARY | L.PHASE_APPLY, True)
        else:
            run(L.PHASE_GATHER)
            if G > 1:
                a2a(sl.table.view(-1), sl.rows.view(-1), None, None, m.group)
            run(L.PHASE_GRADS, True)
            if late:
                plan_late()
            if weight != 1.0:
                scale_by_weight(m, gf, weight)
            if G > 1 and m.coalesce:
                # the two exchanges behind the kernels are independent of each other (the row sums travel unscaled: the
                # clip coefficient reaches the owners through the summary): one RCCL group instead of two collectives
                if _staged(m.group):      # (gloo: no groups of collectives -- the same two exchanges, back to back, in the same place)
                    allreduce_sum(flat, m.group)
                    a2a(self.vals.view(-1), gf.view(-1), None, None, m.group)
                else:
                    with dist._coalescing_manager(group=m.group, device=torch.device(m.device), async_ops=False):
                        dist.all_reduce(flat, group=m.group)
                        dist.all_to_all_single(self.vals.view(-1), gf.view(-1), group=m.group)
                run(L.PHASE_SUMMARY | L.PHASE_APPLY)
            else:
                if G > 1:
                    allreduce_sum(flat, m.group)
                run(L.PHASE_SUMMARY)
                if G > 1:
                    a2a(self.vals.view(-1), gf.view(-1), None, None, m.group)
                run(L.PHASE_APPLY)
        if ahead and capturing:              # a recording must join its forks; eager steps wait where a plan is used
            main.wait_stream(side)
            main.wait_stream(side2)
            for b, kk in ahead:
                slots[kk].joined()
        m._step += 1
        self.prev_stamped = stamp          # (a recorded step never stamps: the step behind a capture or replay takes the event path)
        if not capturing:
            self.warm = True
            if m.renorm_every and m._step % m.renorm_every == 0:
                m.fold_scale()
            if m._step - self.checked >= 1024:
                self.checked = m._step
                self.check_overflow()
        return db

    def capture(self, db, ndb, lr):
        """Record one step in a HIP graph (ShardedModel.capture_step)."""
        m = self.m
        main = self.drain()                                   # nothing of the eager steps is left in flight
        k0, step0 = self.next, m._step
        s0, s1 = self.slots[k0], self.slots[(k0 + 1) % _STATIC_SLOTS]
        for sl in self.slots:
            sl.joined()
        if s0.db is not db or not s0.fresh:                   # the recorded step expects its plan in place
            self._plan(db, k0, main, m.group)
        if m.world > 1 and not self._ids_in_plan(self.side, self.side_group):
            # plans built ahead leave their id exchange to the step that uses them: EVERY replay of this step consumes a
            # plan the previous graph built, so the recording must carry the exchange itself -- whatever the eager plan
            # above has already sent (round 3 recorded g0 without it and replays consumed the first exchange's result)
            s0.ids_sent = False
        if s1.fresh:                                          # (an eager step announced a batch into k1: the graph builds the
            self._discard(s1, main)                           #  next plan itself, every replay -- not on top of that one)
        self._views(s0, db)                                   # ctypes structs are built outside the capture
        self._views(s1, ndb)
        torch.cuda.synchronize(m.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.train(db, lr, ndb, 1.0, 0)
        # recording queues nothing: take the host-side bookkeeping of the step back
        self.next, m._step = k0, step0
        s0.rewind(True)
        s1.rewind(False)
        g._tlsan = (db, ndb, k0, m._ws)
        return g

    def replay(self, g):
        db, ndb, k0, ws = g._tlsan
        m, s0 = self.m, self.slots[k0]
        if ws is not m._ws:
            raise RuntimeError("replay: the workspace was reallocated after this graph was captured; recapture the step")
        if self.next != k0 or s0.db is not db or not s0.fresh or s0.pending:
            raise RuntimeError("replay: this step expects its batch planned in slot %d by the step before it "
                               "(replay the graphs in the order they were captured)" % k0)
        g.replay()
        k1 = (k0 + 1) % _STATIC_SLOTS
        s0.consume()
        self.slots[k1].announce_by_replay(ndb)
        self.next = k1
        self.prev_stamped = False      # (a recorded step carries no stamp: the next eager step orders its plans by an event)
        m._step += 1

"""Collectives and row routing of the row-sharded model (tlsan_amd.dist): the all-to-all / all-reduce / all-gather
wrappers every exchange goes through (host-staged under gloo), and the owner-major key space (`KeyRouter`).

`RowExchange`, `ExchangePlan`, `KeyRouter.plan/fetch/push` and `torch_scan` are the CPU model of the routing (device-agnostic
torch + torch.distributed), exercised by tests/test_dist_cpu.py and used by no product path: all arithmetic on rows is in
libtlsan_hip.so."""
from __future__ import annotations

import torch
import torch.distributed as dist


class ModPartition:
    """Row r of a table with n rows lives on rank r % world at local row r // world."""

    def __init__(self, n, world):
        self.n, self.world = int(n), int(world)

    def local_count(self, rank):
        return (self.n - rank + self.world - 1) // self.world

    def owner(self, ids):
        return ids % self.world

    def local_row(self, ids):
        return torch.div(ids, self.world, rounding_mode="floor")

    def global_ids(self, rank, device=None):
        return torch.arange(rank, self.n, self.world, device=device)


def _staged(group):
    """gloo has no device all-to-all: stage CUDA tensors through the host (used only by the
    single-GPU multi-process tests; RCCL moves device buffers directly)."""
    return dist.get_backend(group) == "gloo"


def a2a(out, inp, out_splits, in_splits, group=None):
    if _staged(group) and out.is_cuda:
        o = torch.empty(out.shape, dtype=out.dtype)
        dist.all_to_all_single(o, inp.cpu().contiguous(), out_splits, in_splits, group=group)
        out.copy_(o)
    else:
        dist.all_to_all_single(out, inp.contiguous(), out_splits, in_splits, group=group)
    return out


def allreduce_sum(t, group=None):
    if _staged(group) and t.is_cuda:
        c = t.cpu()
        dist.all_reduce(c, group=group)
        t.copy_(c)
    else:
        dist.all_reduce(t, group=group)
    return t


def allgather_rows(t, group=None):
    """[n, ...] per rank -> [world * n, ...] in rank order (equal n on every rank)."""
    world = dist.get_world_size(group)
    if world == 1:
        return t
    if _staged(group) and t.is_cuda:
        c = t.cpu().contiguous()
        o = torch.empty((world * c.shape[0],) + tuple(c.shape[1:]), dtype=c.dtype)
        dist.all_gather_into_tensor(o, c, group=group)
        return o.to(t.device)
    o = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(o, t.contiguous(), group=group)
    return o


class ExchangePlan:
    __slots__ = ("order", "send_counts", "recv_counts", "recv_rows", "n")


class RowExchange:
    """Fetch rows of a row-sharded table by global id, and route per-row values back."""

    def __init__(self, part, group=None):
        self.part = part
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        assert self.world == part.world

    def plan(self, uniq_ids):
        """uniq_ids: 1-D int64 tensor of distinct global row ids this rank needs."""
        p = ExchangePlan()
        p.n = int(uniq_ids.numel())
        owner = self.part.owner(uniq_ids)
        p.order = torch.argsort(owner, stable=True)
        ids_sorted = uniq_ids[p.order]
        sc = torch.bincount(owner, minlength=self.world)
        if self.world == 1:
            p.send_counts = [p.n]
            p.recv_counts = [p.n]
            p.recv_rows = self.part.local_row(ids_sorted)
            return p
        rc = torch.empty_like(sc)
        a2a(rc, sc, None, None, self.group)
        p.send_counts = [int(x) for x in sc.tolist()]
        p.recv_counts = [int(x) for x in rc.tolist()]
        recv_ids = torch.empty(sum(p.recv_counts), dtype=uniq_ids.dtype, device=uniq_ids.device)
        a2a(recv_ids, ids_sorted, p.recv_counts, p.send_counts, self.group)
        p.recv_rows = self.part.local_row(recv_ids)
        return p

    def fetch(self, plan, shard):
        """rows of `shard` (this rank's [n_local, width] slice) for every id of the plan, in the
        order of the `uniq_ids` given to plan()."""
        rows = shard[plan.recv_rows]
        if self.world == 1:
            got = rows
        else:
            got = torch.empty((plan.n, shard.shape[1]), dtype=shard.dtype, device=shard.device)
            a2a(got, rows, plan.send_counts, plan.recv_counts, self.group)
        out = torch.empty_like(got)
        out[plan.order] = got
        return out

    def push(self, plan, values):
        """Send one value row per id of the plan back to its owner.  Returns (local_rows, rows):
        contributions concatenated in source-rank order (deterministic)."""
        v = values[plan.order].contiguous()
        if self.world == 1:
            return plan.recv_rows, v
        got = torch.empty((sum(plan.recv_counts), values.shape[1]), dtype=values.dtype, device=values.device)
        a2a(got, v, plan.recv_counts, plan.send_counts, self.group)
        return plan.recv_rows, got


class KeyRouter:
    """Owner-major key space for the fused shard table of one rank group.

    Every rank owns R = cI + cU rows: its items (id % G == rank) at local rows [0, cI) and its
    users at [cI, R).  A global id maps to key = owner * R + local_row, so
      * marking the keys a batch touches and compacting the marks (one scan) yields the distinct
        rows it needs ALREADY grouped by owner, i.e. in all-to-all send order, and the exclusive
        prefix is the id -> compact-row map of the per-step table;
      * what is sent to an owner are its local row numbers (key - owner * R).
    One plan / fetch / push serves both tables: one collective each way instead of two, and no
    sort / unique / bincount kernels."""

    def __init__(self, n_items, n_users, world, rank, group=None):
        self.G, self.rank, self.group = int(world), int(rank), group
        self.cI = (int(n_items) + self.G - 1) // self.G
        self.cU = (int(n_users) + self.G - 1) // self.G
        self.R = self.cI + self.cU
        self.nkeys = self.G * self.R

    def item_keys(self, ids):
        return (ids % self.G) * self.R + torch.div(ids, self.G, rounding_mode="floor")

    def user_keys(self, ids):
        return (ids % self.G) * self.R + self.cI + torch.div(ids, self.G, rounding_mode="floor")

    def plan(self, keys, scan):
        """keys: int64 tensor of every key the batch touches (duplicates fine).  `scan(flags)` ->
        (prefix, uniq, n_uniq_tensor) is the exclusive-scan + compaction primitive
        (tlsan_scan_compact on the GPU).  Returns a dict describing the exchange."""
        dev = keys.device
        flags = torch.zeros(self.nkeys, dtype=torch.int32, device=dev)
        flags[keys] = 1
        prefix, uniq, n_uniq = scan(flags)
        bnd = torch.arange(0, self.nkeys, self.R, device=dev)
        starts = torch.cat([prefix[bnd], n_uniq.reshape(1)])
        sc = (starts[1:] - starts[:-1]).to(torch.int64)
        if self.G > 1:
            rc = torch.empty_like(sc)
            a2a(rc, sc, None, None, self.group)
            both = torch.stack([sc, rc]).cpu()          # the step's single host sync
            send_counts, recv_counts = both[0].tolist(), both[1].tolist()
        else:
            send_counts = recv_counts = sc.cpu().tolist()
        n = int(sum(send_counts))
        uniq = uniq[:n]
        local_rows = uniq % self.R                      # int32 row numbers inside the owner's shard
        if self.G > 1:
            recv_rows = torch.empty(sum(recv_counts), dtype=torch.int32, device=dev)
            a2a(recv_rows, local_rows, recv_counts, send_counts, self.group)
        else:
            recv_rows = local_rows
        return dict(prefix=prefix, uniq=uniq, n=n, send_counts=send_counts, recv_counts=recv_counts,
                    recv_rows=recv_rows)

    def fetch(self, plan, shard):
        """compact per-step table: row k = the shard row of plan['uniq'][k]"""
        rows = shard[plan["recv_rows"].long()]
        if self.G == 1:
            return rows
        out = torch.empty((plan["n"], shard.shape[1]), dtype=shard.dtype, device=shard.device)
        a2a(out, rows, plan["send_counts"], plan["recv_counts"], self.group)
        return out

    def push(self, plan, values):
        """one value row per compact row back to its owner: (local_rows, rows) in source-rank order"""
        if self.G == 1:
            return plan["recv_rows"], values
        got = torch.empty((sum(plan["recv_counts"]), values.shape[1]), dtype=values.dtype, device=values.device)
        a2a(got, values, plan["recv_counts"], plan["send_counts"], self.group)
        return plan["recv_rows"], got


def torch_scan(flags):
    """scan + compaction with torch ops (CPU tests of the routing; the GPU path uses the HIP scan)"""
    inc = torch.cumsum(flags, 0, dtype=torch.int32)
    prefix = inc - flags
    uniq = torch.nonzero(flags, as_tuple=False).reshape(-1).to(torch.int32)
    pad = torch.zeros(flags.numel() - uniq.numel(), dtype=torch.int32, device=flags.device)
    return prefix, torch.cat([uniq, pad]), inc[-1:].clone()

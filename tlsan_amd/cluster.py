"""`ClusteredIndex`: an approximate item index for "the best k over the whole catalogue" -- a partition of the items LEARNED
from their vectors [item_emb || cate_emb[item_cate]] (k-means, tlsan_cluster_assign / tlsan_cluster_means) and, per query,
the choice of the few lists worth scoring (tlsan_cluster_probe).  Everything behind the choice is the indexed lists of a
CategoryIndex as they stand (tlsan_eval_topk_lists / tlsan_similar_topk_lists, tlsan_topk_merge): a returned (row, id, score)
is the exact path's score for that pair bit for bit, a row's list is the exact top k of the union of its probed lists minus
its exclusions, and with probes >= the number of non-empty lists the result IS recommend()'s without an index.  What is
approximate is which lists a row probes, so recall at fewer probes is measured (recall()), never promised: it depends on
how clustered the trained table is (profiles/clustered_index.md)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .model import (CategoryIndex, ItemScope, grow_workspace, item_vectors, lists_similar_topk, lists_topk, topk_merge)

VECTOR_CHUNK = 1 << 18   # item vectors fetched and assigned at a time (a [chunk, d] float32 staging matrix)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def split_lists(assign, ids, nlists, max_list):
    """Cuts the lists of the map assign [item_count] (over the ascending item ids `ids`) that are longer than max_list into
    consecutive chunks of at most max_list ids -> (new map [item_count], parent [L]): chunk lists keep the order of their
    clusters, an empty cluster keeps one (empty) list, parent[l] is the cluster list l came from."""
    a = assign[ids]
    counts = np.bincount(a, minlength=nlists)
    chunks = np.maximum(1, -(-counts // max_list))
    base = np.concatenate([[0], np.cumsum(chunks)])
    order = np.argsort(a, kind="stable")                       # (ids ascend inside a cluster)
    pos = np.arange(len(a)) - np.concatenate([[0], np.cumsum(counts)])[a[order]]
    out = np.zeros_like(assign)
    out[ids[order]] = base[a[order]] + pos // max_list
    return out, np.repeat(np.arange(nlists), chunks)


class ClusteredIndex:
    """A partition of the GLOBAL item ids -- all item_count, or an ItemScope's -- into L lists by nearest centroid, on the
    device: centroids [L, d] float32, list_bias [L] (the mean item_b of a list's items, 0 for an empty list), centroid_inv
    [L] (1 / |centroid|, 0 for a zero one: the cosine metric's scale) and `partition`, a CategoryIndex whose item_cate is
    the item -> list map with cate_count = L (so local(), the sharded-ready layout and max_list are its own).
    Model.cluster_index() trains one; from_assignment() builds one from a given map (tests, device "cpu").

    Training (Lloyd): the training set is min(count, train_size or 256 nlists) ids drawn by np.random.default_rng(seed)
    without replacement and sorted (train_ids), the initial centroids nlists of those rows drawn by the same generator
    (init_ids); an iteration is one assignment, a stable sort by (list, id) with a bincount, and one means call; it stops
    early when no assignment changed.  `objective` holds each iteration's summed squared distance (formed in float64).
    There is no re-seeding: a cluster that loses all its rows keeps its centroid and, if no item comes back to it, ends
    as an empty list, which no probe selects.

    max_list: a list longer than that is cut into consecutive chunks of at most max_list ids, each a list of its own with
    its parent's centroid and bias (`parent` [L] names the cluster) -- the list launch is sized by the longest list.  The
    chunks of one cluster tie in probe score, so they fill consecutive probes: count them when choosing probes=.

    The index is a snapshot of the parameters: rebuild it after training."""

    PROBES = L.CLUSTER_PMAX    # CLUSTER_PMAX (csrc/tlsan_cluster.h): most lists a row probes
    GROUP = CategoryIndex.PROBES   # lists of one tlsan_eval_topk_lists call

    def __init__(self):
        raise TypeError("ClusteredIndex: build one with Model.cluster_index() or ClusteredIndex.from_assignment()")

    @classmethod
    def from_assignment(cls, assign, centroids, device="cpu", item_b=None, within=None, max_list=None):
        """assign [item_count]: the list (cluster) of every item, ids in [0, nlists) (entries outside `within` are not
        looked at beyond that); centroids [nlists, d] float32; item_b [item_count] or None (a zero bias)."""
        a = _host(assign)
        cent = np.ascontiguousarray(_host(centroids), np.float32)
        if cent.ndim != 2 or cent.shape[1] not in (64, 128, 256) or not 1 <= cent.shape[0] <= L.CLUSTER_CMAX:
            raise ValueError("ClusteredIndex: centroids must be [nlists, d], nlists in 1..%d, d 64, 128 or 256, got shape %s"
                             % (L.CLUSTER_CMAX, cent.shape))
        nl = int(cent.shape[0])
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() >= nl)):
            raise ValueError("ClusteredIndex: assign must be a 1-D array of list ids in [0, %d)" % nl)
        a, I = a.astype(np.int64), int(a.shape[0])
        if within is not None and (not isinstance(within, ItemScope) or within.item_count != I):
            raise ValueError("ClusteredIndex: within must be None or an ItemScope over the %d items" % I)
        if max_list is not None and int(max_list) < 1:
            raise ValueError("ClusteredIndex: max_list must be >= 1, got %r" % (max_list,))
        ids = np.arange(I, dtype=np.int64) if within is None else within._host
        parent = np.arange(nl)
        if max_list is not None:
            a, parent = split_lists(a, ids, nl, int(max_list))
            if len(parent) > L.CLUSTER_CMAX:
                raise ValueError("ClusteredIndex: max_list=%d leaves %d lists, more than %d" % (max_list, len(parent), L.CLUSTER_CMAX))
        self = object.__new__(cls)
        self.item_count, self.device, self.within = I, device, within
        self.nlists, self.lists, self.d = nl, int(len(parent)), int(cent.shape[1])
        self.partition = CategoryIndex(a, self.lists, device, within=within)
        self.count, self.max_list = self.partition.count, self.partition.max_list
        sizes = np.bincount(a[ids], minlength=self.lists)
        self.mean_list = float(sizes[sizes > 0].mean()) if self.count else 0.0
        self.nonempty = int((sizes > 0).sum())
        # a cluster's bias: the mean of its items' item_b in float64, in id order, rounded once
        csize = np.bincount(parent, weights=sizes, minlength=nl)
        b = np.zeros(I) if item_b is None else _host(item_b).astype(np.float64).reshape(-1)
        if b.shape != (I,):
            raise ValueError("ClusteredIndex: item_b must be [%d]" % I)
        csum = np.bincount(parent[a[ids]], weights=b[ids], minlength=nl)
        cbias = np.where(csize > 0, csum / np.maximum(csize, 1), 0.0).astype(np.float32)
        norm = np.sqrt((cent.astype(np.float64) ** 2).sum(1))
        cinv = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 0.0).astype(np.float32)
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(device)
        self.parent = dev(parent.astype(np.int32))
        self.centroids = dev(cent[parent])
        self.list_bias = dev(cbias[parent])
        self.centroid_inv = dev(cinv[parent])
        self.train_ids = self.init_ids = None
        self.objective = []
        self._tws = None
        return self

    def probe(self, vectors, P, scale=None, bias=None):
        """row_lists [B, P] int32 (device): the P non-empty lists of highest (v . centroid_j) * scale_j + bias_j for each
        row of vectors [B, d] float32 (tlsan_cluster_probe: higher first, equal -> the lower list, NaN last; -1 in the
        slots that are left over).  scale / bias: [L] float32 device tensors or None (1 / 0).  1 <= P <= 64."""
        P = int(P)
        if not 1 <= P <= self.PROBES:
            raise ValueError("probes must be in 1..%d, got %d" % (self.PROBES, P))
        if torch.device(self.device).type != "cuda":
            raise RuntimeError("ClusteredIndex.probe needs the index on a GPU (no CPU fallback)")
        v = vectors
        if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.shape[1] != self.d or v.dtype != torch.float32 or v.shape[0] < 1 \
                or v.device.type != "cuda":
            raise ValueError("probe: vectors must be a [B, %d] float32 device tensor" % self.d)
        for name, t in (("scale", scale), ("bias", bias)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (self.lists,)
                                  or t.device.type != "cuda"):
                raise ValueError("probe: %s must be a [%d] float32 device tensor" % (name, self.lists))
        lib, B = L.load(), int(v.shape[0])
        v = v.contiguous()
        off = self.partition.local(1, 0, self.item_count)[0]
        nws = lib.tlsan_cluster_workspace_bytes(B, self.lists, P)
        if nws == 0:
            raise L.TlsanError("tlsan_cluster_workspace_bytes: %s" % lib.tlsan_last_error().decode())
        ws = grow_workspace(self, "_tws", nws)
        rows = torch.empty(B, P, dtype=torch.int32, device=v.device)
        ptr = lambda t: None if t is None else t.contiguous().data_ptr()
        L.check(lib.tlsan_cluster_probe(v.data_ptr(), B, self.d, self.centroids.data_ptr(), ptr(scale), ptr(bias), off.data_ptr(),
                                        self.lists, P, rows.data_ptr(), ws.data_ptr(), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream(v.device).cuda_stream)), "tlsan_cluster_probe")
        return rows


def cluster_assign(lib, x, cent, workspace, stream, want_dist=True):
    """tlsan_cluster_assign: x [N, d], cent [C, d] float32 device tensors -> (assign [N] int32, dist [N] float32 or None)."""
    N, d = x.shape
    nc = int(cent.shape[0])
    nws = lib.tlsan_cluster_workspace_bytes(0, nc, 0)
    if nws == 0:
        raise L.TlsanError("tlsan_cluster_workspace_bytes: %s" % lib.tlsan_last_error().decode())
    ws = workspace(nws)
    a = torch.empty(N, dtype=torch.int32, device=x.device)
    dist = torch.empty(N, dtype=torch.float32, device=x.device) if want_dist else None
    L.check(lib.tlsan_cluster_assign(x.data_ptr(), N, d, cent.data_ptr(), nc, a.data_ptr(), None if dist is None else dist.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream), "tlsan_cluster_assign")
    return a, dist


def cluster_means(lib, x, order, seg_off, cent, stream):
    """tlsan_cluster_means: cent[j] <- the mean of x[order[seg_off[j] : seg_off[j + 1]]] (in place; empty: untouched)."""
    L.check(lib.tlsan_cluster_means(x.data_ptr(), int(x.shape[0]), order.data_ptr(), seg_off.data_ptr(), int(cent.shape[0]),
                                    int(x.shape[1]), cent.data_ptr(), stream), "tlsan_cluster_means")


def fit(model, nlists, within=None, iters=10, seed=1234, train_size=None, max_list=None):
    """Model.cluster_index: trains the centroids on the model's item vectors as stored and assigns every item."""
    I = model.config["item_count"]
    nlists, iters = int(nlists), int(iters)
    if not 1 <= nlists <= L.CLUSTER_CMAX:
        raise ValueError("nlists must be in 1..%d, got %d" % (L.CLUSTER_CMAX, nlists))
    if iters < 0:
        raise ValueError("iters must be >= 0, got %d" % iters)
    if within is not None and (not isinstance(within, ItemScope) or within.item_count != I):
        raise ValueError("within must be None or an ItemScope over the model's %d items" % I)
    if max_list is not None and int(max_list) < 1:
        raise ValueError("max_list must be >= 1, got %r" % (max_list,))
    ids = np.arange(I, dtype=np.int64) if within is None else within._host
    n_train = min(len(ids), int(train_size) if train_size is not None else 256 * nlists)
    if n_train < nlists:
        raise ValueError("nlists=%d needs at least as many training items, got %d" % (nlists, n_train))
    rng = np.random.default_rng(seed)
    train_ids = np.sort(rng.choice(ids, n_train, replace=False))
    init_pos = rng.choice(n_train, nlists, replace=False)
    lib, dev = model.lib, model.device
    model._flush()                       # (the vectors are the tables as stored: an owed lazy-L2 correction lands first)
    st = model._stream()
    ws = lambda n: grow_workspace(model, "_tws", n)

    def vectors(some):
        q = torch.as_tensor(some.astype(np.int32)).to(dev)
        return item_vectors(lib, model.dims, model.cparams, q, 1, 0, st)[0]

    x = torch.cat([vectors(train_ids[i:i + VECTOR_CHUNK]) for i in range(0, n_train, VECTOR_CHUNK)])
    cent = x[torch.as_tensor(init_pos).to(dev)].clone()
    pos = torch.arange(n_train, device=dev)
    objective, prev = [], None
    for _ in range(iters):
        a, dist = cluster_assign(lib, x, cent, ws, st)
        objective.append(float(dist.double().sum()))
        if prev is not None and bool(torch.equal(a, prev)):
            break
        prev = a
        order = torch.sort(a.long() * n_train + pos)[1].to(torch.int32)        # (unique keys: by (list, position))
        seg = torch.zeros(nlists + 1, dtype=torch.int32, device=dev)
        seg[1:] = torch.cumsum(torch.bincount(a.long(), minlength=nlists), 0)
        cluster_means(lib, x, order, seg, cent, st)
    del x
    full = np.zeros(I, np.int64)
    for i in range(0, len(ids), VECTOR_CHUNK):
        part = ids[i:i + VECTOR_CHUNK]
        full[part] = cluster_assign(lib, vectors(part), cent, ws, st, want_dist=False)[0].cpu().numpy()
    index = ClusteredIndex.from_assignment(full, cent, dev, item_b=model.item_b, within=within, max_list=max_list)
    index.train_ids, index.init_ids, index.objective = train_ids, train_ids[init_pos], objective
    return index


def clustered_probes(index, probes, item_count, **others):
    """Checks the arguments that go with a ClusteredIndex -> the probe count, or None when `index` is not one (probes= is
    then a ValueError).  others: the arguments that do not go beside a clustered index, by name (None / False: not given)."""
    if not isinstance(index, ClusteredIndex):
        if probes is not None:
            raise ValueError("probes= goes with a ClusteredIndex (cluster_index())")
        return None
    for name, val in others.items():
        if val is not None and val is not False:
            raise ValueError("%s= beside a clustered index: the scope belongs to the index, cluster_index(within=scope)" % name)
    if index.item_count != item_count:
        raise ValueError("index must be a ClusteredIndex over the model's %d items" % item_count)
    if probes is None or isinstance(probes, bool) or int(probes) != probes or not 1 <= int(probes) <= ClusteredIndex.PROBES:
        raise ValueError("a clustered index needs probes= in 1..%d, got %r" % (ClusteredIndex.PROBES, probes))
    return int(probes)


def _grouped(index, rows, run, lib, stream):
    """run(row_lists [B, <= 8]) over ceil(P / 8) groups of a row's probes; more than one group: merged."""
    G = ClusteredIndex.GROUP
    outs = [run(rows[:, g:g + G].contiguous()) for g in range(0, rows.shape[1], G)]
    if len(outs) == 1:
        return outs[0]
    return topk_merge(lib, torch.stack([o[0] for o in outs], 1), torch.stack([o[1] for o in outs], 1), stream)


def clustered_topk(lib, dims, cparams, ut, B, k, excl, index, probes, scale, workspace, stream, boost=None, after=None):
    """recommend's lists with a clustered index on u_t [B, d]: probe (scale: the table scale as [L], or None; bias: the
    lists' mean item_b), then lists_topk per group of 8 probes, then the merge.  boost (model.boost_of's pair): the lists
    are still chosen by the unboosted centroid scores; the scores selected and merged are the boosted ones.  after (the
    rows' model.ListCursor): the probe sees u_t alone, so every page probes the same lists; each group's list is already
    behind the cursor and the merge is unchanged."""
    rows = index.probe(ut, probes, scale=scale, bias=index.list_bias)
    lists = index.partition.local(1, 0, index.item_count)
    return _grouped(index, rows, lambda rl: lists_topk(lib, dims, cparams, ut, B, k, excl, lists, rl, 1, 0, workspace, stream,
                                                            boost=boost, after=after), lib, stream)


def clustered_similar_topk(lib, dims, cparams, vec, inv, qids, k, metric, excl, index, probes, workspace, stream):
    """similar_items' lists with a clustered index: probe on the queries' vectors (cosine: scale 1 / |centroid|; no bias)."""
    rows = index.probe(vec, probes, scale=index.centroid_inv if metric == L.SIM_COSINE else None)
    lists = index.partition.local(1, 0, index.item_count)
    return _grouped(index, rows, lambda rl: lists_similar_topk(lib, dims, cparams, vec, inv, qids, k, metric, excl, lists, rl, 1, 0,
                                                               workspace, stream), lib, stream)


def recall(approx_ids, exact_ids):
    """Mean over the rows of |approx ∩ exact| / |exact| on the valid (>= 0) ids of two [B, k] lists (tensors or arrays);
    rows without a valid exact id are left out (NaN when there is none)."""
    a, e = _host(approx_ids), _host(exact_ids)
    hit = ((a[:, :, None] == e[:, None, :]) & (e[:, None, :] >= 0)).any(1).sum(1)
    n = (e >= 0).sum(1)
    return float((hit[n > 0] / n[n > 0]).mean()) if (n > 0).any() else float("nan")

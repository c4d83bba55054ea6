"""The bf16 shortlist index: recommend's EXACT lists over the whole catalogue in two stages, with a per-row certificate.

Stage 1 (tlsan_shortlist_topk) scans a bf16 snapshot of the item vectors on the bf16 matrix pipe, several 16-row tiles per
loaded item fragment, and keeps each row's N best by approximate score.  Stage 2 scores that shortlist with the exact
path's own scorer (tlsan_score_candidates), picks the k best by exact key and proves, per row, that no item outside the
shortlist can belong to the exact top k (tlsan_shortlist_select; DESIGN.md section 7 has the bound and the proof).  Rows
with the proof are served from the shortlist; the others go through the exact scan (eval_topk) as a sub-batch.  Either way
the caller gets recommend()'s ids and score bits.
    index = model.shortlist_index()
    ids, scores = model.recommend(batch, 10, index=index)            # exact; index.certified says which rows were proven
    ids, scores = model.recommend(batch, 10, index=index, shortlist=128, fallback=False)   # the shortlist's lists as they are
The index is a snapshot of the parameters: rebuild it after training."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


class ShortlistIndex:
    """vec [I, d] bfloat16: [item_emb || cate_emb[item_cate]] as stored, rounded to nearest even (the lazy-L2 scale is not
    folded: it is read at query time); wmax: a [1] float32 device tensor, the largest L2 norm of a stored fp32 row (non-finite
    when an element is).  After a recommend(index=self): certified, the call's [B] bool device tensor; counts, the
    (rows, certified rows) of all calls so far."""

    def __init__(self, vec, wmax):
        self.vec, self.wmax = vec, wmax
        self.item_count, self.d = int(vec.shape[0]), int(vec.shape[1])
        self.device = vec.device
        self.certified = None
        self._counts = torch.zeros(2, dtype=torch.int64, device=vec.device)

    @property
    def counts(self):
        rows, cert = self._counts.tolist()   # (the one host read: nothing is read back per call)
        return rows, cert

    def _count(self, cert):
        self.certified = cert
        self._counts += torch.stack([torch.ones_like(cert, dtype=torch.int64).sum(), cert.sum()])


def build(model):
    """Model.shortlist_index: one launch over the tables as stored (an owed lazy-L2 correction lands first)."""
    model._flush()
    I, d = model.config["item_count"], model.config["hidden_units"]
    vec = torch.empty(I, d, dtype=torch.bfloat16, device=model.device)
    wmax = torch.empty(1, dtype=torch.float32, device=model.device)
    L.check(model.lib.tlsan_shortlist_build(C.byref(model.dims), C.byref(model.cparams), vec.data_ptr(), wmax.data_ptr(),
                                            model._stream()), "tlsan_shortlist_build")
    return ShortlistIndex(vec, wmax)


def default_shortlist(n):
    """The shortlist of a first-stage list of n entries: min(256, max(4 n, 64))."""
    return min(L.SHORTLIST_NMAX, max(4 * int(n), 64))


def shortlist_size(index, shortlist, n, item_count, d, **others):
    """Checks the arguments that go with a ShortlistIndex -> the shortlist length N, or None when `index` is not one
    (shortlist= is then a ValueError).  n: the list length asked of the first stage; others: the arguments that do not go
    beside a shortlist index, by name (None: not given)."""
    if not isinstance(index, ShortlistIndex):
        if shortlist is not None:
            raise ValueError("shortlist= goes with a ShortlistIndex (shortlist_index())")
        return None
    for name, val in others.items():
        if val is not None:
            raise ValueError("%s= beside a shortlist index: it serves the whole catalogue" % name)
    if index.item_count != item_count or index.d != d:
        raise ValueError("index must be a ShortlistIndex over the model's %d items at d = %d" % (item_count, d))
    N = default_shortlist(n) if shortlist is None else shortlist
    if isinstance(N, bool) or int(N) != N or not L.SHORTLIST_NMIN <= int(N) <= L.SHORTLIST_NMAX:
        raise ValueError("shortlist= must be in %d..%d, got %r" % (L.SHORTLIST_NMIN, L.SHORTLIST_NMAX, shortlist))
    if not int(n) < int(N):
        raise ValueError("a list of %d needs a shortlist longer than that, got shortlist=%d" % (n, N))
    return int(N)


def stage1(lib, index, ut, B, N, excl, scale, item_b, ld_itemb, id_mul, id_add, workspace, stream):
    """tlsan_shortlist_topk on u_t [B, d] -> (ids [B, N] int32, approx [B, N] float32).  scale / item_b: device addresses."""
    nws = lib.tlsan_shortlist_workspace_bytes(index.item_count, B, index.d, N)
    if nws == 0:
        raise L.TlsanError(lib.tlsan_last_error().decode())
    ws = workspace(nws)
    ids = torch.empty(B, N, dtype=torch.int32, device=ut.device)
    approx = torch.empty(B, N, dtype=torch.float32, device=ut.device)
    off, xid = excl
    L.check(lib.tlsan_shortlist_topk(index.vec.data_ptr(), index.item_count, index.d, ut.data_ptr(), B, scale, item_b, ld_itemb,
                                     N, None if off is None else off.data_ptr(), None if xid is None else xid.data_ptr(),
                                     id_mul, id_add, ids.data_ptr(), approx.data_ptr(), ws.data_ptr(), ws.numel(), stream),
            "tlsan_shortlist_topk")
    return ids, approx


def select(lib, index, sid, exact, approx, ut, scale, k, stream):
    """tlsan_shortlist_select -> (ids [B, k], scores [B, k], certified [B] int32)."""
    B, N = sid.shape
    ids = torch.empty(B, k, dtype=torch.int32, device=ut.device)
    scores = torch.empty(B, k, dtype=torch.float32, device=ut.device)
    cert = torch.empty(B, dtype=torch.int32, device=ut.device)
    L.check(lib.tlsan_shortlist_select(sid.data_ptr(), exact.data_ptr(), approx.data_ptr(), ut.data_ptr(), scale,
                                       index.wmax.data_ptr(), B, index.d, N, k, ids.data_ptr(), scores.data_ptr(),
                                       cert.data_ptr(), stream), "tlsan_shortlist_select")
    return ids, scores, cert


def excl_rows(excl, rows):
    """The exclusion CSR (excl_off, excl_ids) of the rows `rows` (a 1-D int64 device tensor) of a batch's CSR."""
    off, xid = excl
    if off is None:
        return None, None
    o = off.long()
    lens, starts = (o[1:] - o[:-1])[rows], o[:-1][rows]
    noff = torch.cat([torch.zeros(1, dtype=torch.int64, device=off.device), torch.cumsum(lens, 0)])
    total = int(noff[-1])
    src = torch.repeat_interleave(starts - noff[:-1], lens) + torch.arange(total, device=off.device)
    sub = xid[src] if total else torch.zeros(1, dtype=torch.int32, device=off.device)
    return noff.to(torch.int32), sub.contiguous()


def shortlist_topk(lib, dims, cparams, ut, B, k, excl, index, N, fallback, workspace, stream):
    """recommend's lists of k through a shortlist of N on u_t [B, d]: stage 1, the exact scores of the shortlist, the
    selection and the certificate; with fallback the rows without a certificate (one host read finds them) run through
    eval_topk as a sub-batch and are scattered back.  Leaves the call's certificates in index.certified."""
    from .model import eval_topk, score_candidates
    k = int(k)
    sid, approx = stage1(lib, index, ut, B, N, excl, cparams.scale, cparams.item_b, cparams.ld_itemb or 1, 1, 0, workspace, stream)
    exact = score_candidates(lib, dims, cparams, ut, sid, 1, 0, stream)
    ids, scores, cert = select(lib, index, sid, exact, approx, ut, cparams.scale, k, stream)
    cert = cert != 0
    index._count(cert)
    if fallback:
        rows = (~cert).nonzero().reshape(-1)
        if rows.numel():
            fid, fsc = eval_topk(lib, dims, cparams, ut[rows].contiguous(), int(rows.numel()), k, excl_rows(excl, rows), 1, 0,
                                 workspace, stream)
            ids[rows], scores[rows] = fid, fsc
    return ids, scores

// tlsan_lists_host.h -- the host steps the entry points of the indexed lists share (tlsan_lists.hip: tlsan_lists_workspace_bytes,
// tlsan_eval_topk_lists, tlsan_similar_topk_lists; tlsan_boost.hip: tlsan_eval_topk_lists_boost): the workspace carve-up, the
// refusals, the arguments of the grouping and the fill of the pairs' lists.  The scoring arguments (eval_args) and
// named_refusal are tlsan_scope_host.h's.  Host code only; every function is internal to the unit that includes it.
#pragma once
#include "tlsan_scope_host.h"
#include "tlsan_lists.h"

struct ListsWs {
  int32_t *cnt, *gbase, *ngroups, *rank, *glist, *gpair;
  int32_t* ids;        // [N, nsl, K] the pairs' slice lists (P * nsl > 1)
  float* scores;
  float* inv;          // [I] inv of the index's items, by local item (the cosine form)
  size_t bytes;
  int nsl, ngmax;
};

// the most lists the grouping takes: its scan is one workgroup's, and the counters live in the workspace
#define LISTS_NMAX (1 << 24)

static inline void carve_lists(const tlsan_dims* d, int B, int P, int K, int nlists, int max_list, char* base, ListsWs* w) {
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += al(n); return p; };
  const int N = B * P;
  const int nsl = w->nsl = eval_slices((N + 15) / 16, ((max_list + 63) / 64 + 3) / 4);
  const int ng = w->ngmax = N / 16 + (nlists < N ? nlists : N);
  w->cnt = (int32_t*)take(4 * (size_t)nlists);
  w->gbase = (int32_t*)take(4 * (size_t)nlists);
  w->ngroups = (int32_t*)take(4);
  w->rank = (int32_t*)take(4 * (size_t)N);
  w->glist = (int32_t*)take(4 * (size_t)ng);
  w->gpair = (int32_t*)take(4 * (size_t)ng * 16);
  const size_t nc = P * nsl > 1 ? (size_t)N * nsl * K : 0;
  w->ids = (int32_t*)take(4 * nc);
  w->scores = (float*)take(4 * nc);
  w->inv = (float*)take(sizeof(float) * (size_t)d->item_count);
  w->bytes = o;
}

// what the entries refuse about the scalars (after shape_of: d is a table)
static inline int lists_scalars(const char* fn, int32_t B, int32_t P, int32_t K, int32_t nlists, int32_t max_list) {
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "%s: K must be in 1..%d (got %d)", fn, TOPK_MAX, K);
  if (P < 1 || P > LISTS_PMAX) return fail(TLSAN_E_BADARG, "%s: P must be in 1..%d (got %d)", fn, LISTS_PMAX, P);
  if (B < 1 || B > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: B must be in 1..2^24 (got %d)", fn, B);
  if (nlists < 1 || nlists > LISTS_NMAX) return fail(TLSAN_E_BADARG, "%s: nlists must be in 1..2^24 (got %d)", fn, nlists);
  if (max_list < 0) return fail(TLSAN_E_BADARG, "%s: max_list must be >= 0 (got %d)", fn, max_list);
  return TLSAN_OK;
}

static inline int lists_check(const char* fn, const tlsan_dims* d, int32_t B, int32_t K, const int32_t* excl_off, const int32_t* excl_ids,
                       const int32_t* list_off, const int32_t* list_items, int32_t nlists, const int32_t* row_lists, int32_t P,
                       int32_t max_list, int32_t id_mul, int32_t id_add, void* ws, size_t ws_bytes, ListsWs* w) {
  const int rc = lists_scalars(fn, B, P, K, nlists, max_list);
  if (rc) return rc;
  if (!list_off || !list_items || !row_lists) return fail(TLSAN_E_BADARG, "%s: list_off, list_items or row_lists is NULL", fn);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "%s: excl_off and excl_ids go together", fn);
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "%s: global ids n * id_mul + id_add must be non-negative int32", fn);
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  carve_lists(d, B, P, K, nlists, max_list, (char*)ws, w);
  if (w->bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, w->bytes, ws_bytes);
  return TLSAN_OK;
}

static inline ListsArgs lists_args(const ListsWs& w, const int32_t* list_off, const int32_t* list_items, int32_t nlists,
                            const int32_t* row_lists, int32_t B, int32_t P) {
  ListsArgs l;
  memset(&l, 0, sizeof(l));
  l.list_off = list_off; l.list_items = list_items; l.row_lists = row_lists; l.nlists = nlists; l.P = P; l.N = B * P;
  l.cnt = w.cnt; l.gbase = w.gbase; l.ngroups = w.ngroups; l.rank = w.rank; l.glist = w.glist; l.gpair = w.gpair;
  return l;
}

// every slot of the lists the scan writes into: id -1, score -inf
static inline hipError_t lists_fill(int32_t* ids, float* scores, size_t n, hipStream_t hs) {
  hipError_t err = hipMemsetD32Async((hipDeviceptr_t)ids, -1, n, hs);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)scores, (int)0xff800000u, n, hs);
  return err;
}

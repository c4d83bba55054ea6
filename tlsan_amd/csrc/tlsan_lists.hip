// Indexed lists (tlsan_lists.h): the instantiations, their launches and the three entry points of the C ABI
// (include/tlsan.h: tlsan_lists_workspace_bytes, tlsan_eval_topk_lists, tlsan_similar_topk_lists).  The merge of a row's
// lists is tlsan_topk.hip's k_topk_merge.
#include <stdio.h>

#include "tlsan_host.h"
#include "tlsan_lists.h"

static hipError_t launch_lists_group(const ListsArgs& l, hipStream_t hs) {
  const dim3 grid((l.N + 255) / 256);
  const hipError_t err = hipMemsetAsync(l.cnt, 0, sizeof(int32_t) * (size_t)l.nlists, hs);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_lists_count, grid, dim3(256), 0, hs, l);
  hipLaunchKernelGGL(k_lists_groups, dim3(1), dim3(1024), 0, hs, l);
  hipLaunchKernelGGL(k_lists_place, grid, dim3(256), 0, hs, l);
  return hipGetLastError();
}

static hipError_t launch_lists_topk(const ListsTopkArgs& a, int D, int ngroups, int nslices, hipStream_t hs) {
  const dim3 grid(ngroups, nslices);
  dispatch_d(D, [&](auto d) {
#define LISTS_L(KP, BUF) hipLaunchKernelGGL((k_lists_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.t.K, LISTS_L);
#undef LISTS_L
  });
  return hipGetLastError();
}

static hipError_t launch_lists_similar(const ListsSimArgs& a, int D, int ngroups, int nslices, hipStream_t hs) {
  const dim3 grid(ngroups, nslices);
  dispatch_d(D, [&](auto d) {
#define LISTS_L(KP, BUF) hipLaunchKernelGGL((k_lists_similar<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.m.t.K, LISTS_L);
#undef LISTS_L
  });
  return hipGetLastError();
}

static hipError_t launch_lists_inv(const EvalArgs& e, const ListsArgs& l, int D, float* inv, hipStream_t hs) {
  const int want = (e.I + 15) / 16;
  const dim3 grid(want < 8192 ? want : 8192);
  dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(k_lists_inv<d.value>, grid, dim3(256), 0, hs, e, l, inv); });
  return hipGetLastError();
}

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

static void carve_lists(const tlsan_dims* d, int B, int P, int K, int nlists, int max_list, char* base, ListsWs* w) {
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

// a refusal of shape_of / check_params, with the entry point's name in front of its message
static int lists_named(const char* fn, int rc) {
  char m[384];
  snprintf(m, sizeof(m), "%s", tlsan_last_error());
  return fail(rc, "%s: %s", fn, m);
}

// what the three entries refuse about the scalars (after shape_of: d is a table)
static int lists_scalars(const char* fn, int32_t B, int32_t P, int32_t K, int32_t nlists, int32_t max_list) {
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "%s: K must be in 1..%d (got %d)", fn, TOPK_MAX, K);
  if (P < 1 || P > LISTS_PMAX) return fail(TLSAN_E_BADARG, "%s: P must be in 1..%d (got %d)", fn, LISTS_PMAX, P);
  if (B < 1 || B > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: B must be in 1..2^24 (got %d)", fn, B);
  if (nlists < 1 || nlists > LISTS_NMAX) return fail(TLSAN_E_BADARG, "%s: nlists must be in 1..2^24 (got %d)", fn, nlists);
  if (max_list < 0) return fail(TLSAN_E_BADARG, "%s: max_list must be >= 0 (got %d)", fn, max_list);
  return TLSAN_OK;
}

static int lists_check(const char* fn, const tlsan_dims* d, int32_t B, int32_t K, const int32_t* excl_off, const int32_t* excl_ids,
                       const int32_t* list_off, const int32_t* list_items, int32_t nlists, const int32_t* row_lists, int32_t P,
                       int32_t max_list, int32_t id_mul, int32_t id_add, void* ws, size_t ws_bytes, ListsWs* w) {
  const int rc = lists_scalars(fn, B, P, K, nlists, max_list);
  if (rc) return rc;
  if (!list_off || !list_items || !row_lists) return fail(TLSAN_E_BADARG, "%s: list_off, list_items or row_lists is NULL", fn);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "%s: excl_off and excl_ids go together", fn);
  if (!(id_mul >= 1 && id_add >= 0 && (long long)(d->item_count - 1) * id_mul + id_add < (1LL << 31)))
    return fail(TLSAN_E_BADARG, "%s: global ids n * id_mul + id_add must be non-negative int32", fn);
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  carve_lists(d, B, P, K, nlists, max_list, (char*)ws, w);
  if (w->bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, w->bytes, ws_bytes);
  return TLSAN_OK;
}

static EvalArgs lists_eval_args(const tlsan_dims* d, const tlsan_params* p, const float* rows, int32_t B, int32_t id_mul, int32_t id_add) {
  EvalArgs e;
  memset(&e, 0, sizeof(e));
  e.p = norm_params(p, d); e.u_t = rows; e.B = B; e.I = d->item_count; e.di = d->d_item; e.dc = d->d_cate;
  e.id_mul = id_mul; e.id_add = id_add;          // (all_emb stays NULL: the gather form)
  return e;
}

static ListsArgs lists_args(const ListsWs& w, const int32_t* list_off, const int32_t* list_items, int32_t nlists,
                            const int32_t* row_lists, int32_t B, int32_t P) {
  ListsArgs l;
  memset(&l, 0, sizeof(l));
  l.list_off = list_off; l.list_items = list_items; l.row_lists = row_lists; l.nlists = nlists; l.P = P; l.N = B * P;
  l.cnt = w.cnt; l.gbase = w.gbase; l.ngroups = w.ngroups; l.rank = w.rank; l.glist = w.glist; l.gpair = w.gpair;
  return l;
}

// every slot of the lists the scan writes into: id -1, score -inf
static hipError_t lists_fill(int32_t* ids, float* scores, size_t n, hipStream_t hs) {
  hipError_t err = hipMemsetD32Async((hipDeviceptr_t)ids, -1, n, hs);
  if (err == hipSuccess) err = hipMemsetD32Async((hipDeviceptr_t)scores, (int)0xff800000u, n, hs);
  return err;
}

extern "C" {

size_t tlsan_lists_workspace_bytes(const tlsan_dims* d, int32_t B, int32_t P, int32_t K, int32_t nlists, int32_t max_list) {
  static const char* fn = "tlsan_lists_workspace_bytes";
  Shape s;
  const int rc = shape_of(d, &s);
  if (rc) { lists_named(fn, rc); return 0; }
  if (lists_scalars(fn, B, P, K, nlists, max_list)) return 0;
  ListsWs w;
  carve_lists(d, B, P, K, nlists, max_list, nullptr, &w);
  return w.bytes;
}

int tlsan_eval_topk_lists(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                          const int32_t* excl_off, const int32_t* excl_ids, const int32_t* list_off, const int32_t* list_items,
                          int32_t nlists, int32_t max_list, const int32_t* row_lists, int32_t P, int32_t id_mul, int32_t id_add,
                          int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_eval_topk_lists";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return lists_named(fn, rc);
  if (!u_t || !ids || !scores) return fail(TLSAN_E_BADARG, "%s: u_t, ids or scores is NULL", fn);
  ListsWs w;
  if ((rc = lists_check(fn, d, B, K, excl_off, excl_ids, list_off, list_items, nlists, row_lists, P, max_list, id_mul, id_add, ws,
                        ws_bytes, &w)))
    return rc;
  hipStream_t hs = (hipStream_t)stream;
  const int nl = P * w.nsl;
  ListsTopkArgs la;
  memset(&la, 0, sizeof(la));
  TopkArgs& ta = la.t;
  ta.e = lists_eval_args(d, p, u_t, B, id_mul, id_add);
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nl > 1 ? w.ids : ids;
  ta.scores = nl > 1 ? w.scores : scores;
  la.l = lists_args(w, list_off, list_items, nlists, row_lists, B, P);
  hipError_t err = launch_lists_group(la.l, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s: the grouping: %s", fn, hipGetErrorString(err));
  if ((err = lists_fill(ta.ids, ta.scores, (size_t)B * nl * K, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "%s: the fill: %s", fn, hipGetErrorString(err));
  if ((err = launch_lists_topk(la, s.D, w.ngmax, w.nsl, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_lists_topk: %s", hipGetErrorString(err));
  if (nl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, nl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_similar_topk_lists(const tlsan_dims* d, const tlsan_params* p, const float* qvec, const float* qinv, const int32_t* qids,
                             int32_t Q, int32_t K, int32_t metric, const int32_t* excl_off, const int32_t* excl_ids,
                             const int32_t* list_off, const int32_t* list_items, int32_t nlists, int32_t max_list,
                             const int32_t* row_lists, int32_t P, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores,
                             void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_similar_topk_lists";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return lists_named(fn, rc);
  if (metric != SIM_DOT && metric != SIM_COSINE)
    return fail(TLSAN_E_BADARG, "%s: metric must be TLSAN_SIM_DOT or TLSAN_SIM_COSINE (got %d)", fn, metric);
  if (!qvec || !qids || !ids || !scores || (metric == SIM_COSINE && !qinv)) return fail(TLSAN_E_BADARG, "%s: NULL argument", fn);
  ListsWs w;
  if ((rc = lists_check(fn, d, Q, K, excl_off, excl_ids, list_off, list_items, nlists, row_lists, P, max_list, id_mul, id_add, ws,
                        ws_bytes, &w)))
    return rc;
  hipStream_t hs = (hipStream_t)stream;
  const int nl = P * w.nsl;
  ListsSimArgs la;
  memset(&la, 0, sizeof(la));
  TopkArgs& ta = la.m.t;
  ta.e = lists_eval_args(d, p, qvec, Q, id_mul, id_add);
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nl > 1 ? w.ids : ids;
  ta.scores = nl > 1 ? w.scores : scores;
  la.m.qinv = qinv; la.m.qids = qids; la.m.inv = w.inv; la.m.metric = metric;
  la.l = lists_args(w, list_off, list_items, nlists, row_lists, Q, P);
  hipError_t err = launch_lists_group(la.l, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s: the grouping: %s", fn, hipGetErrorString(err));
  if ((err = lists_fill(ta.ids, ta.scores, (size_t)Q * nl * K, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "%s: the fill: %s", fn, hipGetErrorString(err));
  if (metric == SIM_COSINE && (err = launch_lists_inv(ta.e, la.l, s.D, w.inv, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_lists_inv: %s", hipGetErrorString(err));
  if ((err = launch_lists_similar(la, s.D, w.ngmax, w.nsl, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_lists_similar: %s", hipGetErrorString(err));
  if (nl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, Q, nl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

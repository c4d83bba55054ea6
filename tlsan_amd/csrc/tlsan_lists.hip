// Indexed lists (tlsan_lists.h): the grouping kernels with their launcher (tlsan_launch_lists_group, which the boosted call
// of tlsan_boost.hip shares), the instantiations, their launches and the three entry points of the C ABI
// (include/tlsan.h: tlsan_lists_workspace_bytes, tlsan_eval_topk_lists, tlsan_similar_topk_lists).  The checks and the
// workspace carve-up are tlsan_lists_host.h's; the merge of a row's lists is tlsan_topk.hip's k_topk_merge.
#include <stdio.h>

#include "tlsan_host.h"
#include "tlsan_lists.h"
#include "tlsan_lists_host.h"

// The grouping of the valid (row, probe) pairs by list (tlsan_lists.h says what a group is).
__global__ __launch_bounds__(256) void k_lists_count(ListsArgs l) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= l.N) return;
  const int b0 = t - t % l.P;
  const int c = l.row_lists[t];
  bool ok = (unsigned)c < (unsigned)l.nlists;          // (a list id past the index is no probe: list_off is not addressed)
  for (int j = b0; j < t; ++j) ok = ok && l.row_lists[j] != c;
  if (ok) ok = l.list_off[c + 1] > l.list_off[c];
  l.rank[t] = ok ? atomicAdd(&l.cnt[c], 1) : -1;
}

__global__ __launch_bounds__(1024) void k_lists_groups(ListsArgs l) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int per = (l.nlists + 1023) / 1024;
  const int lo = min(t * per, l.nlists), hi = min(lo + per, l.nlists);
  int s = 0;
  for (int c = lo; c < hi; ++c) s += (l.cnt[c] + 15) >> 4;
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = part[t] - s;
  for (int c = lo; c < hi; ++c) {
    l.gbase[c] = base;
    base += (l.cnt[c] + 15) >> 4;
  }
  if (t == 1023) l.ngroups[0] = part[1023];
}

__global__ __launch_bounds__(256) void k_lists_place(ListsArgs l) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= l.N) return;
  const int rk = l.rank[t];
  if (rk < 0) return;
  const int c = l.row_lists[t];
  const int g = l.gbase[c] + (rk >> 4);
  l.gpair[(size_t)g * 16 + (rk & 15)] = t;
  if ((rk & 15) == 0) l.glist[g] = c;
}

hipError_t tlsan_launch_lists_group(const ListsArgs& l, hipStream_t hs) {
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

extern "C" {

size_t tlsan_lists_workspace_bytes(const tlsan_dims* d, int32_t B, int32_t P, int32_t K, int32_t nlists, int32_t max_list) {
  static const char* fn = "tlsan_lists_workspace_bytes";
  Shape s;
  const int rc = shape_of(d, &s);
  if (rc) { named_refusal(fn, rc); return 0; }
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
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
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
  ta.e = eval_args(d, p, u_t, B, id_mul, id_add);
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nl > 1 ? w.ids : ids;
  ta.scores = nl > 1 ? w.scores : scores;
  la.l = lists_args(w, list_off, list_items, nlists, row_lists, B, P);
  hipError_t err = tlsan_launch_lists_group(la.l, hs);
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
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
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
  ta.e = eval_args(d, p, qvec, Q, id_mul, id_add);
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nl > 1 ? w.ids : ids;
  ta.scores = nl > 1 ? w.scores : scores;
  la.m.qinv = qinv; la.m.qids = qids; la.m.inv = w.inv; la.m.metric = metric;
  la.l = lists_args(w, list_off, list_items, nlists, row_lists, Q, P);
  hipError_t err = tlsan_launch_lists_group(la.l, hs);
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

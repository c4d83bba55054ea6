// Lists behind a cursor (tlsan_after.h): the instantiations, their launches and the three entry points of the C ABI
// (include/tlsan.h: tlsan_eval_topk_scoped_after, tlsan_eval_topk_lists_after, tlsan_dense_topk_after).  The checks, the
// workspaces and the launch geometry are the twins' without a cursor (tlsan_scope_host.h, tlsan_lists_host.h,
// tlsan_dense_host.h); the grouping of an indexed call is tlsan_lists.hip's and the merge of a row's lists tlsan_topk.hip's
// k_topk_merge, which needs no cursor: every slice's list is already behind it.
#include "tlsan_host.h"
#include "tlsan_after.h"
#include "tlsan_dense_host.h"
#include "tlsan_lists_host.h"

static hipError_t launch_after_scoped(const AfterScopedArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.s.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define AFTER_L(KP, BUF) hipLaunchKernelGGL((k_after_scoped_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.s.t.K, AFTER_L);
#undef AFTER_L
  });
  return hipGetLastError();
}

static hipError_t launch_after_lists(const AfterListsArgs& a, int D, int ngroups, int nslices, hipStream_t hs) {
  const dim3 grid(ngroups, nslices);
  dispatch_d(D, [&](auto d) {
#define AFTER_L(KP, BUF) hipLaunchKernelGGL((k_after_lists_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.l.t.K, AFTER_L);
#undef AFTER_L
  });
  return hipGetLastError();
}

static hipError_t launch_after_dense(const AfterDenseArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.d.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define AFTER_L(KP, BUF) hipLaunchKernelGGL((k_after_dense_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.d.t.K, AFTER_L);
#undef AFTER_L
  });
  return hipGetLastError();
}

// the refusals about the cursor and the boost that the three calls share (twin: the call without a cursor)
static int after_check(const char* fn, const char* twin, const int32_t* after_ids, const float* after_scores, const float* boost,
                       const float* row_weight) {
  if (!after_ids || !after_scores)
    return fail(TLSAN_E_BADARG, "%s: after_ids or after_scores is NULL (%s is the call without a cursor)", fn, twin);
  if (row_weight && !boost) return fail(TLSAN_E_BADARG, "%s: row_weight weighs boost: boost is NULL", fn);
  return TLSAN_OK;
}

extern "C" {

int tlsan_eval_topk_scoped_after(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                 const int32_t* excl_off, const int32_t* excl_ids, const int32_t* sub, int32_t nsub,
                                 const int32_t* row_cate, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                                 size_t ws_bytes, void* stream, const float* boost, const float* row_weight,
                                 const int32_t* after_ids, const float* after_scores) {
  static const char* fn = "tlsan_eval_topk_scoped_after";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!u_t || !ids || !scores || B < 1) return fail(TLSAN_E_BADARG, "%s: bad arguments", fn);
  if ((rc = after_check(fn, boost ? "tlsan_eval_topk_scoped_boost" : "tlsan_eval_topk_scoped", after_ids, after_scores, boost,
                        row_weight)))
    return rc;
  ScopeWs w;
  if ((rc = scope_check(fn, d, B, K, excl_off, excl_ids, sub, nsub, id_mul, id_add, ws, ws_bytes, &w))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  AfterScopedArgs aa;
  memset(&aa, 0, sizeof(aa));
  TopkArgs& ta = aa.s.t;
  ta.e = eval_args(d, p, u_t, B, id_mul, id_add);      // (all_emb stays NULL: the gather form)
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = w.nsl > 1 ? w.ids : ids;
  ta.scores = w.nsl > 1 ? w.scores : scores;
  aa.s.s.sub = sub; aa.s.s.nsub = nsub < 0 ? 0 : nsub; aa.s.s.row_cate = row_cate;
  aa.b.boost = boost; aa.b.row_weight = row_weight;
  aa.c.ids = after_ids; aa.c.scores = after_scores;
  hipError_t err = launch_after_scoped(aa, s.D, w.nsl, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_after_scoped_topk: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_eval_topk_lists_after(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                const int32_t* excl_off, const int32_t* excl_ids, const int32_t* list_off, const int32_t* list_items,
                                int32_t nlists, int32_t max_list, const int32_t* row_lists, int32_t P, int32_t id_mul, int32_t id_add,
                                int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream, const float* boost,
                                const float* row_weight, const int32_t* after_ids, const float* after_scores) {
  static const char* fn = "tlsan_eval_topk_lists_after";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!u_t || !ids || !scores) return fail(TLSAN_E_BADARG, "%s: u_t, ids or scores is NULL", fn);
  if ((rc = after_check(fn, boost ? "tlsan_eval_topk_lists_boost" : "tlsan_eval_topk_lists", after_ids, after_scores, boost,
                        row_weight)))
    return rc;
  ListsWs w;
  if ((rc = lists_check(fn, d, B, K, excl_off, excl_ids, list_off, list_items, nlists, row_lists, P, max_list, id_mul, id_add, ws,
                        ws_bytes, &w)))
    return rc;
  hipStream_t hs = (hipStream_t)stream;
  const int nl = P * w.nsl;
  AfterListsArgs aa;
  memset(&aa, 0, sizeof(aa));
  TopkArgs& ta = aa.l.t;
  ta.e = eval_args(d, p, u_t, B, id_mul, id_add);      // (all_emb stays NULL: the gather form)
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nl > 1 ? w.ids : ids;
  ta.scores = nl > 1 ? w.scores : scores;
  aa.l.l = lists_args(w, list_off, list_items, nlists, row_lists, B, P);
  aa.b.boost = boost; aa.b.row_weight = row_weight;
  aa.c.ids = after_ids; aa.c.scores = after_scores;
  hipError_t err = tlsan_launch_lists_group(aa.l.l, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s: the grouping: %s", fn, hipGetErrorString(err));
  if ((err = lists_fill(ta.ids, ta.scores, (size_t)B * nl * K, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "%s: the fill: %s", fn, hipGetErrorString(err));
  if ((err = launch_after_lists(aa, s.D, w.ngmax, w.nsl, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_after_lists_topk: %s", hipGetErrorString(err));
  if (nl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, nl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_dense_topk_after(const float* q, int32_t Q, int32_t d, const float* x, int32_t N, const float* q_scale, const float* q_bias,
                           const int32_t* excl_off, const int32_t* excl_ids, int32_t id_add, int32_t K, int32_t* ids, float* scores,
                           void* ws, size_t ws_bytes, void* stream, const int32_t* after_ids, const float* after_scores) {
  static const char* fn = "tlsan_dense_topk_after";
  int rc;
  DenseWs w;
  if ((rc = dense_check(fn, q, Q, d, x, N, excl_off, excl_ids, id_add, K, ids, scores, ws, ws_bytes, &w))) return rc;
  if ((rc = after_check(fn, "tlsan_dense_topk", after_ids, after_scores, nullptr, nullptr))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  AfterDenseArgs aa;
  aa.d = dense_args(q, Q, x, N, q_scale, q_bias, excl_off, excl_ids, id_add, K, ids, scores, w);
  aa.c.ids = after_ids; aa.c.scores = after_scores;
  hipError_t err = launch_after_dense(aa, d, w.nsl, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_after_dense_topk: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, Q, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

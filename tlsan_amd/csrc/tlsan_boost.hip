// Boosted lists (tlsan_boost.h): the instantiations, their launches and the two entry points of the C ABI (include/tlsan.h:
// tlsan_eval_topk_scoped_boost, tlsan_eval_topk_lists_boost).  The checks, the workspaces and the launch geometry are the
// unboosted calls' (tlsan_scope_host.h, tlsan_lists_host.h); the grouping of an indexed call is tlsan_lists.hip's and the
// merge of a row's lists tlsan_topk.hip's k_topk_merge.
#include "tlsan_host.h"
#include "tlsan_boost.h"
#include "tlsan_lists_host.h"

static hipError_t launch_boost_scoped(const BoostedScopedArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.s.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define BOOST_L(KP, BUF) hipLaunchKernelGGL((k_boost_scoped_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.s.t.K, BOOST_L);
#undef BOOST_L
  });
  return hipGetLastError();
}

static hipError_t launch_boost_lists(const BoostedListsArgs& a, int D, int ngroups, int nslices, hipStream_t hs) {
  const dim3 grid(ngroups, nslices);
  dispatch_d(D, [&](auto d) {
#define BOOST_L(KP, BUF) hipLaunchKernelGGL((k_boost_lists_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.l.t.K, BOOST_L);
#undef BOOST_L
  });
  return hipGetLastError();
}

extern "C" {

int tlsan_eval_topk_scoped_boost(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                 const int32_t* excl_off, const int32_t* excl_ids, const int32_t* sub, int32_t nsub,
                                 const int32_t* row_cate, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                                 size_t ws_bytes, void* stream, const float* boost, const float* row_weight) {
  static const char* fn = "tlsan_eval_topk_scoped_boost";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!u_t || !ids || !scores || B < 1) return fail(TLSAN_E_BADARG, "%s: bad arguments", fn);
  if (!boost) return fail(TLSAN_E_BADARG, "%s: boost is NULL (tlsan_eval_topk_scoped is the call without one)", fn);
  ScopeWs w;
  if ((rc = scope_check(fn, d, B, K, excl_off, excl_ids, sub, nsub, id_mul, id_add, ws, ws_bytes, &w))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  BoostedScopedArgs ba;
  memset(&ba, 0, sizeof(ba));
  TopkArgs& ta = ba.s.t;
  ta.e = eval_args(d, p, u_t, B, id_mul, id_add);      // (all_emb stays NULL: the gather form)
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = w.nsl > 1 ? w.ids : ids;
  ta.scores = w.nsl > 1 ? w.scores : scores;
  ba.s.s.sub = sub; ba.s.s.nsub = nsub < 0 ? 0 : nsub; ba.s.s.row_cate = row_cate;
  ba.b.boost = boost; ba.b.row_weight = row_weight;
  hipError_t err = launch_boost_scoped(ba, s.D, w.nsl, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_boost_scoped_topk: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_eval_topk_lists_boost(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                const int32_t* excl_off, const int32_t* excl_ids, const int32_t* list_off, const int32_t* list_items,
                                int32_t nlists, int32_t max_list, const int32_t* row_lists, int32_t P, int32_t id_mul, int32_t id_add,
                                int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream, const float* boost,
                                const float* row_weight) {
  static const char* fn = "tlsan_eval_topk_lists_boost";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!u_t || !ids || !scores) return fail(TLSAN_E_BADARG, "%s: u_t, ids or scores is NULL", fn);
  if (!boost) return fail(TLSAN_E_BADARG, "%s: boost is NULL (tlsan_eval_topk_lists is the call without one)", fn);
  ListsWs w;
  if ((rc = lists_check(fn, d, B, K, excl_off, excl_ids, list_off, list_items, nlists, row_lists, P, max_list, id_mul, id_add, ws,
                        ws_bytes, &w)))
    return rc;
  hipStream_t hs = (hipStream_t)stream;
  const int nl = P * w.nsl;
  BoostedListsArgs ba;
  memset(&ba, 0, sizeof(ba));
  TopkArgs& ta = ba.l.t;
  ta.e = eval_args(d, p, u_t, B, id_mul, id_add);      // (all_emb stays NULL: the gather form)
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nl > 1 ? w.ids : ids;
  ta.scores = nl > 1 ? w.scores : scores;
  ba.l.l = lists_args(w, list_off, list_items, nlists, row_lists, B, P);
  ba.b.boost = boost; ba.b.row_weight = row_weight;
  hipError_t err = tlsan_launch_lists_group(ba.l.l, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s: the grouping: %s", fn, hipGetErrorString(err));
  if ((err = lists_fill(ta.ids, ta.scores, (size_t)B * nl * K, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "%s: the fill: %s", fn, hipGetErrorString(err));
  if ((err = launch_boost_lists(ba, s.D, w.ngmax, w.nsl, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_boost_lists_topk: %s", hipGetErrorString(err));
  if (nl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, nl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

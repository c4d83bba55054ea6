// The dense top-K call (tlsan_dense.h): the instantiations, their launch and the two entry points of the C ABI
// (include/tlsan.h: tlsan_dense_topk_workspace_bytes, tlsan_dense_topk) with their argument checks.  The call reads no
// table, so nothing of the other host units is needed but fail() and the merge's launcher (tlsan_topk.hip's k_topk_merge).
// The checks and the workspace are tlsan_dense_host.h's, shared with the call behind a cursor (tlsan_after.hip).
#include "tlsan_dense_host.h"

static hipError_t launch_dense_topk(const DenseTopkArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define DENSE_L(KP, BUF) hipLaunchKernelGGL((k_dense_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.t.K, DENSE_L);
#undef DENSE_L
  });
  return hipGetLastError();
}

extern "C" {

size_t tlsan_dense_topk_workspace_bytes(int32_t Q, int32_t N, int32_t K) {
  if (dense_sizes("tlsan_dense_topk_workspace_bytes", Q, N, K)) return 0;
  DenseWs w;
  carve_dense(Q, N, K, nullptr, &w);
  return w.bytes;
}

int tlsan_dense_topk(const float* q, int32_t Q, int32_t d, const float* x, int32_t N, const float* q_scale, const float* q_bias,
                     const int32_t* excl_off, const int32_t* excl_ids, int32_t id_add, int32_t K, int32_t* ids, float* scores,
                     void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_dense_topk";
  int rc;
  DenseWs w;
  if ((rc = dense_check(fn, q, Q, d, x, N, excl_off, excl_ids, id_add, K, ids, scores, ws, ws_bytes, &w))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  const DenseTopkArgs da = dense_args(q, Q, x, N, q_scale, q_bias, excl_off, excl_ids, id_add, K, ids, scores, w);
  hipError_t err = launch_dense_topk(da, d, w.nsl, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_dense_topk: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, Q, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

// Scoped lists (tlsan_scope.h): the instantiations and their launches.  Arguments are checked by the callers in
// tlsan_api_eval.hip (tlsan_eval_topk_scoped, tlsan_similar_topk_scoped).
#include "tlsan_scope.h"

hipError_t tlsan_launch_scoped_topk(const ScopedTopkArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define SCOPE_L(KP, BUF) hipLaunchKernelGGL((k_scoped_topk<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.t.K, SCOPE_L);
#undef SCOPE_L
  });
  return hipGetLastError();
}

hipError_t tlsan_launch_scoped_similar(const ScopedSimArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.m.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define SCOPE_L(KP, BUF) hipLaunchKernelGGL((k_scoped_similar<d.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(a.m.t.K, SCOPE_L);
#undef SCOPE_L
  });
  return hipGetLastError();
}

// count >= 1 positions (the caller launches nothing for an empty scope)
hipError_t tlsan_launch_scope_inv(const EvalArgs& e, const ScopeArgs& s, int count, int D, float* inv, hipStream_t hs) {
  const dim3 grid((count + 15) / 16);
  dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(k_scope_inv<d.value>, grid, dim3(256), 0, hs, e, s, inv); });
  return hipGetLastError();
}

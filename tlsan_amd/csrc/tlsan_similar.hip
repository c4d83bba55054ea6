// Similar-items lists (tlsan_similar.h): the instantiations and their launches.  Arguments are checked by the callers in
// tlsan_api_eval.hip (tlsan_item_vectors, tlsan_similar_topk).
#include "tlsan_similar.h"

hipError_t tlsan_launch_similar_topk(const SimArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.t.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define SIM_L(KP, BUF)                                                                                         \
  do {                                                                                                         \
    if (a.t.e.all_emb) hipLaunchKernelGGL((k_similar_topk<d.value, KP, BUF, true>), grid, dim3(256), 0, hs, a); \
    else hipLaunchKernelGGL((k_similar_topk<d.value, KP, BUF, false>), grid, dim3(256), 0, hs, a);              \
  } while (0)
    TOPK_DISPATCH(a.t.K, SIM_L);
#undef SIM_L
  });
  return hipGetLastError();
}

hipError_t tlsan_launch_sim_prep(const EvalArgs& e, int D, float* inv, hipStream_t hs) {
  const dim3 grid((e.I + 15) / 16);
  dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(k_sim_prep<d.value>, grid, dim3(256), 0, hs, e, inv); });
  return hipGetLastError();
}

hipError_t tlsan_launch_item_vectors(const VecArgs& a, int D, hipStream_t hs) {
  const dim3 grid((a.Q + 15) / 16);
  dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(k_item_vectors<d.value>, grid, dim3(256), 0, hs, a); });
  return hipGetLastError();
}

// Top-K selection over all items (tlsan_topk.h): the instantiations and their launches.  Arguments are checked by the
// callers in tlsan_api_eval.hip (tlsan_eval_topk, tlsan_topk_merge).
#include "tlsan_topk.h"

hipError_t tlsan_launch_topk(const TopkArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.e.B + 15) / 16, nslices);
  dispatch_d(D, [&](auto d) {
#define TOPK_L(KP, BUF)                                                                                    \
  do {                                                                                                     \
    if (a.e.all_emb) hipLaunchKernelGGL((k_eval_topk<d.value, KP, BUF, true>), grid, dim3(256), 0, hs, a); \
    else hipLaunchKernelGGL((k_eval_topk<d.value, KP, BUF, false>), grid, dim3(256), 0, hs, a);            \
  } while (0)
    TOPK_DISPATCH(a.K, TOPK_L);
#undef TOPK_L
  });
  return hipGetLastError();
}

hipError_t tlsan_launch_topk_merge(const int32_t* cid, const float* csc, int B, int nl, int K, int32_t* ids,
                                   float* scores, hipStream_t hs) {
  const dim3 grid((B + 15) / 16);
#define TOPK_M(KP, BUF) hipLaunchKernelGGL((k_topk_merge<KP, BUF>), grid, dim3(256), 0, hs, cid, csc, B, nl, K, ids, scores)
  TOPK_DISPATCH(K, TOPK_M);
#undef TOPK_M
  return hipGetLastError();
}

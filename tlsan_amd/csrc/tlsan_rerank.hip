// Diversified lists (tlsan_rerank.h): the instantiations and their launch.  Arguments are checked by the caller in
// tlsan_api_eval.hip (tlsan_rerank).
#include "tlsan_rerank.h"

hipError_t tlsan_launch_rerank(const RerankArgs& a, int D, hipStream_t hs) {
  dispatch_d(D, [&](auto d) {
    if (a.N <= 64) hipLaunchKernelGGL((k_rerank<d.value, 256>), dim3(a.B), dim3(256), 0, hs, a);
    else hipLaunchKernelGGL((k_rerank<d.value, 1024>), dim3(a.B), dim3(1024), 0, hs, a);
  });
  return hipGetLastError();
}

// Similar-items lists (tlsan_similar.h): the instantiations and their launches.  Arguments are checked by the callers in
// tlsan_api_eval.hip (tlsan_item_vectors, tlsan_similar_topk).
#include "tlsan_similar.h"

// (kept list, append buffer) per query by K: the classes of TOPK_DISPATCH (tlsan_topk.hip), whose LDS budget this is
#define SIM_DISPATCH(K, F) \
  do {                       \
    if ((K) <= 16) F(16, 128); \
    else if ((K) <= 64) F(64, 128); \
    else F(256, 256);          \
  } while (0)

template <int D>
static void launch_similar(const SimArgs& a, dim3 grid, hipStream_t hs) {
#define SIM_L(KP, BUF)                                                                                  \
  do {                                                                                                  \
    if (a.t.e.all_emb) hipLaunchKernelGGL((k_similar_topk<D, KP, BUF, true>), grid, dim3(256), 0, hs, a); \
    else hipLaunchKernelGGL((k_similar_topk<D, KP, BUF, false>), grid, dim3(256), 0, hs, a);              \
  } while (0)
  SIM_DISPATCH(a.t.K, SIM_L);
#undef SIM_L
}

hipError_t tlsan_launch_similar_topk(const SimArgs& a, int D, int nslices, hipStream_t hs) {
  const dim3 grid((a.t.e.B + 15) / 16, nslices);
  if (D == 64) launch_similar<64>(a, grid, hs);
  else if (D == 128) launch_similar<128>(a, grid, hs);
  else launch_similar<256>(a, grid, hs);
  return hipGetLastError();
}

hipError_t tlsan_launch_sim_prep(const EvalArgs& e, int D, float* inv, hipStream_t hs) {
  const dim3 grid((e.I + 15) / 16);
  if (D == 64) hipLaunchKernelGGL(k_sim_prep<64>, grid, dim3(256), 0, hs, e, inv);
  else if (D == 128) hipLaunchKernelGGL(k_sim_prep<128>, grid, dim3(256), 0, hs, e, inv);
  else hipLaunchKernelGGL(k_sim_prep<256>, grid, dim3(256), 0, hs, e, inv);
  return hipGetLastError();
}

hipError_t tlsan_launch_item_vectors(const VecArgs& a, int D, hipStream_t hs) {
  const dim3 grid((a.Q + 15) / 16);
  if (D == 64) hipLaunchKernelGGL(k_item_vectors<64>, grid, dim3(256), 0, hs, a);
  else if (D == 128) hipLaunchKernelGGL(k_item_vectors<128>, grid, dim3(256), 0, hs, a);
  else hipLaunchKernelGGL(k_item_vectors<256>, grid, dim3(256), 0, hs, a);
  return hipGetLastError();
}

// List metrics (tlsan_listm.h): the instantiations, their launch and the entry point tlsan_list_metrics with its argument
// checks -- the call reads no table, so nothing of the other host units is needed but fail().
#include "tlsan_host.h"
#include "tlsan_listm.h"

hipError_t tlsan_launch_list_metrics(const ListmArgs& a, int D, hipStream_t hs) {
  dispatch_d(D, [&](auto d) {
    if (a.K <= 64) hipLaunchKernelGGL((k_list_metrics<d.value, 256>), dim3(a.B), dim3(256), 0, hs, a);
    else hipLaunchKernelGGL((k_list_metrics<d.value, 1024>), dim3(a.B), dim3(1024), 0, hs, a);
  });
  return hipGetLastError();
}

extern "C" int tlsan_list_metrics(const int32_t* ids, const float* vec, const float* inv, const int32_t* cate,
                                  const int32_t* labels, const float* weight, int32_t B, int32_t K, int32_t d,
                                  int32_t* n_valid, double* pair_cos, int32_t* n_cate, int32_t* max_cate, int32_t* hit_pos,
                                  double* weight_sum, uint32_t* exposure, int32_t n_items, void* stream) {
  if (K < 1 || K > LISTM_MAX) return fail(TLSAN_E_BADARG, "tlsan_list_metrics: K must be in 1..%d (got %d)", LISTM_MAX, K);
  if (d != 64 && d != 128 && d != 256)
    return fail(TLSAN_E_UNSUPPORTED, "tlsan_list_metrics: d must be 64, 128 or 256 (got %d)", d);
  if (B < 1 || (long long)B * K >= (1LL << 31))
    return fail(TLSAN_E_BADARG, "tlsan_list_metrics: B must be >= 1 and B * K below 2^31 (got B %d, K %d)", B, K);
  if (exposure && n_items < 1)
    return fail(TLSAN_E_BADARG, "tlsan_list_metrics: exposure needs n_items >= 1 (got %d)", n_items);
  if (!ids || !vec || !inv || !cate || !n_valid || !pair_cos || !n_cate || !max_cate || !hit_pos || !weight_sum)
    return fail(TLSAN_E_BADARG, "tlsan_list_metrics: NULL argument");
  ListmArgs a;
  memset(&a, 0, sizeof(a));
  a.ids = ids; a.vec = vec; a.inv = inv; a.cate = cate; a.labels = labels; a.weight = weight;
  a.B = B; a.K = K; a.n_items = exposure ? n_items : 0;
  a.n_valid = n_valid; a.pair_cos = pair_cos; a.n_cate = n_cate; a.max_cate = max_cate; a.hit_pos = hit_pos;
  a.weight_sum = weight_sum; a.exposure = exposure;
  const hipError_t err = tlsan_launch_list_metrics(a, d, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_list_metrics: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

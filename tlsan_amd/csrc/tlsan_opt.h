// tlsan_opt.h -- what the row updates of every optimizer step share, one model's (tlsan_apply.h) or a row shard's
// (tlsan_shard.h): the fixed-order block sum of doubles and the element rule of Adam / RMSProp / Adadelta.
#pragma once
#include "tlsan_common.h"

// fixed-order sum of doubles by one 256-thread block
__device__ __forceinline__ double block_sum_double(const double* __restrict__ v, int n, double* sh) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k0 = tid; k0 < n; k0 += 256 * 8) {  // 8 loads in flight (clamped addresses, masked sum)
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = v[k0 + 256 * u < n ? k0 + 256 * u : k0];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += k0 + 256 * u < n ? t[u] : 0.0;
  }
  sh[tid] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  return sh[0];
}

// One element under TF 1.8's Adam / RMSProp / Adadelta (training_ops.cc; the Sparse* forms are the
// same arithmetic per row).  g: clipped gradient of the parameter; s1, s2: its two accumulators.
struct OptCtx {
  int opt;
  float lr, b1, b2, eps, alpha;
};
__device__ __forceinline__ void opt_elem(const OptCtx& o, float& w, float g, float& s1, float& s2) {
  if (o.opt == TLSAN_OPT_ADAM) {
    s1 = s1 * o.b1 + g * (1.0f - o.b1);
    s2 = s2 * o.b2 + (g * g) * (1.0f - o.b2);
    w -= o.alpha * s1 / (sqrtf(s2) + o.eps);
  } else if (o.opt == TLSAN_OPT_RMSPROP) {  // b1 = decay, b2 = momentum
    s1 = s1 * o.b1 + (g * g) * (1.0f - o.b1);
    s2 = s2 * o.b2 + o.lr * g / sqrtf(s1 + o.eps);
    w -= s2;
  } else {  // Adadelta, b1 = rho
    s1 = s1 * o.b1 + (g * g) * (1.0f - o.b1);
    const float upd = sqrtf(s2 + o.eps) / sqrtf(s1 + o.eps) * g;
    w -= upd * o.lr;
    s2 = s2 * o.b1 + (upd * upd) * (1.0f - o.b1);
  }
}

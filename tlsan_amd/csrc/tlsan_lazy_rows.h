// tlsan_lazy_rows.h -- the category rows of a lazy-L2 SGD update from their presummed gradients: what the split form's
// second launch (k_update_lazy, tlsan_update_lazy.h) and k_spec_commit<.., CSPL> (tlsan_spec_commit.h) share.
#pragma once
#include "tlsan_apply.h"

// 16 category rows, one per 16-lane group: w -= lazy_scale * (the row's presummed gradient: Rc, or Rc64 -- the exact doubles the
// split category workgroups left, rounded to float as a single workgroup would have, and cleared).  Returns the lane's share
// of the change of the stored table's sum of squares.  (k_update_lazy; k_spec_commit<.., CSPL>)
template <int NC, int DT>
__device__ __forceinline__ double update_cate_rows(const ApplyArgs& a, int c, int l16, float lazy_scale, uint32_t salt) {
  double part = 0.0;
  if (c < a.C) {
    const size_t wrow = (size_t)c * a.dc;
    f32x4 w[NC], g[NC];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
      if (4 * (l16 + 16 * ch) < a.dc) {
        w[ch] = tbl_ld4<DT>(a.p.cate_emb, wrow + 4 * (l16 + 16 * ch));
        if (a.csplit > 1) {
          double* r64 = a.Rc64 + wrow + 4 * (l16 + 16 * ch);
#pragma unroll
          for (int i = 0; i < 4; ++i) { g[ch][i] = (float)r64[i]; r64[i] = 0.0; }
        } else {
          g[ch] = *(const f32x4*)(a.Rc + wrow + 4 * (l16 + 16 * ch));
        }
      }
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
      if (4 * (l16 + 16 * ch) < a.dc) {
        const f32x4 w0 = w[ch];
        w[ch] = w0 - lazy_scale * g[ch];
        tbl_st4<DT>(a.p.cate_emb, wrow + 4 * (l16 + 16 * ch), w[ch], salt ^ 0x3c6ef372u);
#pragma unroll
        for (int i = 0; i < 4; ++i) part += (double)w[ch][i] * (double)w[ch][i] - (double)w0[i] * (double)w0[i];
      }
  }
  return part;
}

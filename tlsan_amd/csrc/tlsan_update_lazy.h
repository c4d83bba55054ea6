// tlsan_update_lazy.h -- the kernels behind the finalize that only tlsan_api.hip launches: the second launch of the split
// lazy step (k_update_lazy, and k_update_lazy_opt for the lazy optimizers), the float copy of the split category sums
// (k_rc64_to_float) and tlsan_state_renorm's kernels.
#pragma once
#include "tlsan_lazy_rows.h"

// split category sums (Rc64, exact doubles) -> float output, and back to zero at rest (tlsan_grads)
__global__ void k_rc64_to_float(double* __restrict__ r64, float* __restrict__ out, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    out[t] = (float)r64[t];
    r64[t] = 0.0;
  }
}

// grid: nbC16 = ceil(C / 16) blocks of category rows, nbI / nbU blocks of used item / user rows
// (one row per 16-lane group), nbD blocks of 256 dense parameters
template <bool WIDE, int DT>
__global__ __launch_bounds__(256) void k_update_lazy(ApplyArgs a, int nbC16) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  __shared__ double shp[4];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, gid = tid >> 4, blk = blockIdx.x;
  const float P = a.hdr->P_prev;  // (the step summary already advanced hdr->P)
  const float step = a.lr * a.hdr->coef;
  const float lazy_scale = step / (P * (1.0f - step * a.reg));
  const uint32_t salt = a.hdr->nstep;
  if (blk == 0 && tid == 0) a.hdr->spart_n[salt & 1] = nbC16 + a.nbI + a.nbU;
  double part = 0.0;
  if (blk < nbC16) {
    part = update_cate_rows<NC, DT>(a, blk * 16 + gid, l16, lazy_scale, salt);
  } else if (blk < nbC16 + a.nbI) {
    const int slot0 = (blk - nbC16) * AP_ROWS_PB, slot = slot0 + gid;
    const int nuq = *a.n_uniq_item;
    if (slot0 >= nuq) return;
    if (slot < nuq) {
      const int row = a.urec_item[slot].x;
      const size_t wrow = (size_t)row * a.p.ld_item;
      f32x4 w[NI], g[NI];
      float wb = 0.0f, gb = 0.0f;
#pragma unroll
      for (int ch = 0; ch < NI; ++ch)
        if (4 * (l16 + 16 * ch) < a.di) {
          w[ch] = tbl_ld4<DT>(a.p.item_emb, wrow + 4 * (l16 + 16 * ch));
          g[ch] = *(const f32x4*)(a.Ri + (size_t)slot * a.di + 4 * (l16 + 16 * ch));
        }
      if (l16 == 0) { wb = a.p.item_b[(size_t)row * a.p.ld_itemb]; gb = a.Rb[slot]; }
#pragma unroll
      for (int ch = 0; ch < NI; ++ch)
        if (4 * (l16 + 16 * ch) < a.di) {
          const f32x4 w0 = w[ch];
          w[ch] = w0 - lazy_scale * g[ch];
          tbl_st4<DT>(a.p.item_emb, wrow + 4 * (l16 + 16 * ch), w[ch], salt ^ 0x85ebca6bu);
#pragma unroll
          for (int i = 0; i < 4; ++i) part += (double)w[ch][i] * (double)w[ch][i] - (double)w0[i] * (double)w0[i];
        }
      if (l16 == 0) a.p.item_b[(size_t)row * a.p.ld_itemb] = wb - step * gb;  // not regularised, never scaled
    }
  } else if (blk < nbC16 + a.nbI + a.nbU) {
    const int slot0 = (blk - nbC16 - a.nbI) * AP_ROWS_PB, slot = slot0 + gid;
    const int nuq = *a.n_uniq_user;
    if (slot0 >= nuq) return;
    if (slot < nuq) {
      const int row = a.urec_user[slot].x;
      const size_t wrow = (size_t)row * a.p.ld_user;
      float* Trow = a.p.usert_emb + (size_t)row * a.p.ld_usert;
      f32x4 w[NU], g[NU];
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.WU) g[ch] = *(const f32x4*)(a.Ru + (size_t)slot * a.WU + cc);
        if (cc < a.di) {
          w[ch] = tbl_ld4<DT>(a.p.user_emb, wrow + cc);
        } else if (cc < a.WU) {
#pragma unroll
          for (int i = 0; i < 4; ++i) w[ch][i] = (cc + i - a.di < a.Ls) ? Trow[cc + i - a.di] : 0.0f;
        }
      }
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          const f32x4 w0 = w[ch];
          w[ch] = w0 - lazy_scale * g[ch];
          tbl_st4<DT>(a.p.user_emb, wrow + cc, w[ch], salt ^ 0xc2b2ae35u);
#pragma unroll
          for (int i = 0; i < 4; ++i) part += (double)w[ch][i] * (double)w[ch][i] - (double)w0[i] * (double)w0[i];
        } else if (cc < a.WU) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int p = cc + i - a.di;
            if (p < a.Ls) {
              const float w0 = w[ch][i], wn = w0 - lazy_scale * g[ch][i];
              Trow[p] = wn;
              part += (double)wn * (double)wn - (double)w0 * (double)w0;
            }
          }
        }
      }
    }
  } else {
    const int nd = (blk - nbC16 - a.nbI - a.nbU) * 256 + tid;
    if (nd < a.lay.n_dense) dense_store(a, nd, a.p.dense[nd] - step * a.gd[nd]);
    return;
  }
  block_delta_store(part, shp, a, blk, salt);
}

// ------------------------------------------------------------------------------------------
// Lazy Adam / RMSProp / Adadelta (TLSAN_OPT_LAZY): the split tail's second launch for those optimizers, in place of
// k_update_lazy.  The dense optimizer's step restricted to the rows the batch used: a used row gets opt_elem with
// g = coef * (R + reg * P w) -- R its exact gradient sum (Rc / Rc64 / Ri / Ru, left by k_finalize_presum) -- on the row's
// true values P w and its two slots, the result stored as (P w)' / P; every other row keeps W and both slots bit for bit.
// The finalize does not commit the table scale, so P stays as it is: 1 under these optimizers from the start (then P w is
// w and the step is the dense form's for that row, bit for bit), something else only if lazy-L2 SGD steps ran on the
// same state before.
//   category rows: used when the index counts a use in the category's segment (its u_cate uses; with category segments,
//                  every use) or when the row's summed gradient has a non-zero element (the uses through its items, which
//                  have no count of their own without segments; a row whose gradient sums to exactly zero is left alone).
//                  Every category row's sum is read; W and the slots only of the used rows
//   item / user rows: the index's used-row records; item_b moves where its summed gradient is non-zero (the candidates)
//   dense parameters: every one, as in k_apply
// Same block layout, S_delta records and spart_n protocol as k_update_lazy; split category sums are cleared as there.

// The step's scalars
struct LazyOptCtx {
  OptCtx oc;
  float coef, reg, P, invP;   // clip coefficient, L2 rate, table scale and its inverse
};

// one element of a regularised table: stored value w, true value P w
__device__ __forceinline__ float opt_elem_scaled(const LazyOptCtx& x, float w0, float r, float& s1, float& s2) {
  float wt = x.P * w0;
  opt_elem(x.oc, wt, x.coef * (r + x.reg * (x.P * w0)), s1, s2);
  return wt * x.invP;
}

// four elements of a regularised row and of its slots: returns the change of the stored elements' sum of squares
template <int DT>
__device__ __forceinline__ double opt_row4(const LazyOptCtx& x, float* W, size_t widx, const f32x4& w0, const f32x4& r,
                                           f32x4& m1, f32x4& m2, uint32_t stream) {
  f32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a1 = m1[i], a2 = m2[i];
    w[i] = opt_elem_scaled(x, w0[i], r[i], a1, a2);
    m1[i] = a1; m2[i] = a2;
  }
  tbl_st4<DT>(W, widx, w, stream);
  double part = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) part += (double)w[i] * (double)w[i] - (double)w0[i] * (double)w0[i];
  return part;
}

// 16 category rows, one per 16-lane group (k_update_lazy_opt)
template <int NC, int DT>
__device__ __forceinline__ double update_cate_rows_opt(const ApplyArgs& a, const LazyOptCtx& x, int c, int lane,
                                                       uint32_t salt) {
  const int l16 = lane & 15;
  const bool vc = c < a.C;
  const size_t wrow = (size_t)(vc ? c : 0) * a.dc;
  f32x4 w[NC], g[NC], m1[NC], m2[NC];
  // (the same for the 16 lanes of the row: a row the index counts as used has its W and slots requested beside its sum)
  const bool counted = vc && a.off_uc[c + 1] > a.off_uc[c];
  bool nz = counted;
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
    const size_t e = wrow + 4 * (l16 + 16 * ch);
    if (vc && 4 * (l16 + 16 * ch) < a.dc) {
      if (counted) {
        w[ch] = tbl_ld4<DT>(a.p.cate_emb, e);
        m1[ch] = *(const f32x4*)(a.s1.cate_emb + e);
        m2[ch] = *(const f32x4*)(a.s2.cate_emb + e);
      }
      if (a.csplit > 1) {
        double* r64 = a.Rc64 + e;
#pragma unroll
        for (int i = 0; i < 4; ++i) { g[ch][i] = (float)r64[i]; r64[i] = 0.0; }
      } else {
        g[ch] = *(const f32x4*)(a.Rc + e);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) nz = nz || g[ch][i] != 0.0f;
    }
  }
  const bool used = ((__ballot(nz) >> (lane & 48)) & 0xffffull) != 0;   // any lane of the row's 16-lane group
  double part = 0.0;
  if (used) {
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {   // (the rows reached through their items only: W and slots once the sum is known)
      const size_t e = wrow + 4 * (l16 + 16 * ch);
      if (!counted && 4 * (l16 + 16 * ch) < a.dc) {
        w[ch] = tbl_ld4<DT>(a.p.cate_emb, e);
        m1[ch] = *(const f32x4*)(a.s1.cate_emb + e);
        m2[ch] = *(const f32x4*)(a.s2.cate_emb + e);
      }
    }
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      const size_t e = wrow + 4 * (l16 + 16 * ch);
      if (4 * (l16 + 16 * ch) < a.dc) {
        part += opt_row4<DT>(x, a.p.cate_emb, e, w[ch], g[ch], m1[ch], m2[ch], salt ^ 0x3c6ef372u);
        *(f32x4*)(a.s1.cate_emb + e) = m1[ch];
        *(f32x4*)(a.s2.cate_emb + e) = m2[ch];
      }
    }
  }
  return part;
}

// grid: nbC16 = ceil(C / 16) blocks of category rows, nbI / nbU blocks of used item / user rows
// (one row per 16-lane group), nbD blocks of 256 dense parameters
template <bool WIDE, int DT>
__global__ __launch_bounds__(256) void k_update_lazy_opt(ApplyArgs a, int nbC16) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  __shared__ double shp[4];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, gid = tid >> 4, blk = blockIdx.x;
  LazyOptCtx x;
  x.oc.opt = a.opt; x.oc.lr = a.lr; x.oc.b1 = a.ob1; x.oc.b2 = a.ob2; x.oc.eps = a.oeps; x.oc.alpha = a.oalpha;
  x.coef = a.hdr->coef;
  x.reg = a.reg;
  x.P = a.hdr->P;   // (not committed by this step's finalize)
  x.invP = 1.0f / x.P;
  const OptCtx& oc = x.oc;
  const float coef = x.coef;
  const uint32_t salt = a.hdr->nstep;
  if (blk == 0 && tid == 0) a.hdr->spart_n[salt & 1] = nbC16 + a.nbI + a.nbU;
  double part = 0.0;
  if (blk < nbC16) {
    part = update_cate_rows_opt<NC, DT>(a, x, blk * 16 + gid, lane, salt);
  } else if (blk < nbC16 + a.nbI) {
    const int slot0 = (blk - nbC16) * AP_ROWS_PB, slot = slot0 + gid;
    const int nuq = *a.n_uniq_item;
    if (slot0 >= nuq) return;
    if (slot < nuq) {
      const int row = a.urec_item[slot].x;
      const size_t wrow = (size_t)row * a.p.ld_item;
      float* S1 = a.s1.item_emb + (size_t)row * a.s1.ld_item;
      float* S2 = a.s2.item_emb + (size_t)row * a.s2.ld_item;
      f32x4 w[NI], g[NI], m1[NI], m2[NI];
      float wb = 0.0f, gb = 0.0f;
#pragma unroll
      for (int ch = 0; ch < NI; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          w[ch] = tbl_ld4<DT>(a.p.item_emb, wrow + cc);
          g[ch] = *(const f32x4*)(a.Ri + (size_t)slot * a.di + cc);
          m1[ch] = *(const f32x4*)(S1 + cc);
          m2[ch] = *(const f32x4*)(S2 + cc);
        }
      }
      if (l16 == 0) { wb = a.p.item_b[(size_t)row * a.p.ld_itemb]; gb = a.Rb[slot]; }
#pragma unroll
      for (int ch = 0; ch < NI; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          part += opt_row4<DT>(x, a.p.item_emb, wrow + cc, w[ch], g[ch], m1[ch], m2[ch], salt ^ 0x85ebca6bu);
          *(f32x4*)(S1 + cc) = m1[ch];
          *(f32x4*)(S2 + cc) = m2[ch];
        }
      }
      if (l16 == 0 && gb != 0.0f) {   // item_b: not regularised; moves where the candidates gave it a gradient (k_apply)
        float* q1 = a.s1.item_b + (size_t)row * a.s1.ld_itemb;
        float* q2 = a.s2.item_b + (size_t)row * a.s2.ld_itemb;
        float a1 = *q1, a2 = *q2;
        opt_elem(oc, wb, coef * gb, a1, a2);
        a.p.item_b[(size_t)row * a.p.ld_itemb] = wb;
        *q1 = a1; *q2 = a2;
      }
    }
  } else if (blk < nbC16 + a.nbI + a.nbU) {
    const int slot0 = (blk - nbC16 - a.nbI) * AP_ROWS_PB, slot = slot0 + gid;
    const int nuq = *a.n_uniq_user;
    if (slot0 >= nuq) return;
    if (slot < nuq) {
      const int row = a.urec_user[slot].x;
      const size_t wrow = (size_t)row * a.p.ld_user;
      float* S1 = a.s1.user_emb + (size_t)row * a.s1.ld_user;
      float* S2 = a.s2.user_emb + (size_t)row * a.s2.ld_user;
      float* Trow = a.p.usert_emb + (size_t)row * a.p.ld_usert;
      float* T1 = a.s1.usert_emb + (size_t)row * a.s1.ld_usert;
      float* T2 = a.s2.usert_emb + (size_t)row * a.s2.ld_usert;
      f32x4 w[NU], g[NU], m1[NU], m2[NU];
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.WU) g[ch] = *(const f32x4*)(a.Ru + (size_t)slot * a.WU + cc);
        if (cc < a.di) {
          w[ch] = tbl_ld4<DT>(a.p.user_emb, wrow + cc);
          m1[ch] = *(const f32x4*)(S1 + cc);
          m2[ch] = *(const f32x4*)(S2 + cc);
        } else if (cc < a.WU) {   // usert_emb columns (scalar: Ls need not be a multiple of 4)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int p = cc + i - a.di;
            const bool in = p < a.Ls;
            w[ch][i] = in ? Trow[p] : 0.0f;
            m1[ch][i] = in ? T1[p] : 0.0f;
            m2[ch][i] = in ? T2[p] : 0.0f;
          }
        }
      }
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          part += opt_row4<DT>(x, a.p.user_emb, wrow + cc, w[ch], g[ch], m1[ch], m2[ch], salt ^ 0xc2b2ae35u);
          *(f32x4*)(S1 + cc) = m1[ch];
          *(f32x4*)(S2 + cc) = m2[ch];
        } else if (cc < a.WU) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int p = cc + i - a.di;
            if (p < a.Ls) {
              const float w0 = w[ch][i];
              float a1 = m1[ch][i], a2 = m2[ch][i];
              const float wn = opt_elem_scaled(x, w0, g[ch][i], a1, a2);
              Trow[p] = wn; T1[p] = a1; T2[p] = a2;
              part += (double)wn * (double)wn - (double)w0 * (double)w0;
            }
          }
        }
      }
    }
  } else {
    const int nd = (blk - nbC16 - a.nbI - a.nbU) * 256 + tid;
    if (nd < a.lay.n_dense) {
      float wn = a.p.dense[nd], a1 = a.s1.dense[nd], a2 = a.s2.dense[nd];
      opt_elem(oc, wn, coef * a.gd[nd], a1, a2);
      a.s1.dense[nd] = a1; a.s2.dense[nd] = a2;
      dense_store(a, nd, wn);
    }
    return;
  }
  block_delta_store(part, shp, a, blk, salt);
}

// stored *= P for one table (tlsan_state_renorm)
// (dt: storage type of the table; width % 4 == 0 for bf16 tables; bf16 values are rounded stochastically)
__global__ void k_scale_table(float* W, int rows, int width, int ld, const StateHdr* hdr, int dt, uint32_t salt) {
  const float P = hdr->P;
  if (dt == TLSAN_TABLE_F32) {
    const size_t n = (size_t)rows * width;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
      const size_t r = t / width, c = t % width;
      W[r * ld + c] *= P;
    }
    return;
  }
  const size_t n4 = (size_t)rows * (width / 4);
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += (size_t)gridDim.x * blockDim.x) {
    const size_t r = t / (width / 4), c = 4 * (t % (width / 4));
    f32x4 w = tbl_ld4<TLSAN_TABLE_BF16>(W, r * ld + c) * P;
    tbl_st4<TLSAN_TABLE_BF16>(W, r * ld + c, w, salt ^ hdr->nstep);
  }
}

__global__ void k_renorm_commit(StateHdr* hdr) {
  const double P = hdr->P;
  hdr->St *= P * P;
  hdr->P = 1.0f;
}

// tlsan_update_adagrad.h -- lazy Adagrad and row-wise Adagrad (TLSAN_OPT_ADAGRAD / TLSAN_OPT_ROWWISE_ADAGRAD with
// TLSAN_OPT_LAZY): the split tail's second launch for those two kinds, in place of k_update_lazy_opt, which only
// tlsan_api.hip launches.  Everything but the rule is k_update_lazy_opt's (tlsan_update_lazy.h): a used row gets
// g = coef * (R + reg * P w) -- R its exact gradient sum -- on its true values P w, stored as (P w)' / P; every other row
// keeps W and its accumulator bit for bit; the same used-row rules, block layout, request order, S_delta records, spart_n
// protocol, clearing of the split category sums and bf16 salts.
//   rule (TF 1.8's ApplyAdagrad, no epsilon):  acc += g^2;  w -= lr * g / sqrt(acc)
//   elementwise: one accumulator per element -- slot1 shaped like the parameters
//   row-wise:    one accumulator per row of item_emb / user_emb / usert_emb / cate_emb -- slot1's tables are [rows] floats;
//                acc_row += (1 / n) * sum_j g_j^2 over the row's n live columns (d_item, d_item, Ls, d_cate), then every
//                column steps with the new acc_row.  item_b and the dense weights (width 1) take the elementwise rule in
//                both forms: on a row of width 1 the two rules are the same arithmetic.
// The row sum is not elementwise, which opt_elem cannot express.  Its order is fixed: a lane adds the squares of its own
// live elements in ascending column order (fp32), then the row's 16 lanes combine in four DPP steps (group16_sum) -- no LDS,
// no atomics, nothing that depends on arrival order: two runs leave the same bits.
#pragma once
#include "tlsan_lazy_rows.h"

// The step's scalars
struct AdagradCtx {
  float lr, coef, reg, P, invP;   // learning rate, clip coefficient, L2 rate, table scale and its inverse
};

// one accumulator and the step it gives: returns the new value of w (item_b, dense weights, and the elementwise form's elements)
__device__ __forceinline__ float adagrad_elem(float lr, float w, float g, float& acc) {
  acc += g * g;
  return w - lr * g / sqrtf(acc);
}

// Sum over the 16 lanes of a row's group (a DPP row; all 16 active), the same bits in every lane: lanes_sum<16>
// (tlsan_common.h), the xor butterfly 1, 2, 4, 8 in four DPP moves of the vector ALU.  Steps 1 and 2 are quad permutes; after
// them the four lanes of a quad hold the same bits (a + b == b + a), so the partner lane ^ 4 may be any lane of the half's other
// quad -- row_half_mirror -- and likewise lane ^ 8 any lane of the other half -- row_mirror (gfx9 has no DPP xor mask).
// __shfl_xor would be four ds_bpermute round trips through the LDS unit with a wait each.
__device__ __forceinline__ float group16_sum(float v) { return lanes_sum<16>(v); }

// the clipped gradient of four elements of a regularised row (stored w0, summed gradient r), in place of r; their squares
// join the lane's sum ss one by one, in ascending order
__device__ __forceinline__ void adagrad_grad4(const AdagradCtx& x, const f32x4& w0, f32x4& r, float& ss) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    r[i] = x.coef * (r[i] + x.reg * (x.P * w0[i]));
    ss += r[i] * r[i];
  }
}

// one element of a regularised table from its clipped gradient g: elementwise, acc is the element's accumulator (updated);
// row-wise, the row's NEW accumulator (kept).  Returns the stored value.
template <bool ROWWISE>
__device__ __forceinline__ float adagrad_scaled(const AdagradCtx& x, float w0, float g, float& acc) {
  float wt = x.P * w0;
  if constexpr (ROWWISE) wt -= x.lr * g / sqrtf(acc);
  else wt = adagrad_elem(x.lr, wt, g, acc);
  return wt * x.invP;
}

// four elements of a regularised row: stores them, returns the change of the stored elements' sum of squares
template <int DT, bool ROWWISE>
__device__ __forceinline__ double adagrad_row4(const AdagradCtx& x, float* W, size_t widx, const f32x4& w0, const f32x4& g,
                                               f32x4& m, float acc_row, uint32_t stream) {
  f32x4 w;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float acc = ROWWISE ? acc_row : m[i];
    w[i] = adagrad_scaled<ROWWISE>(x, w0[i], g[i], acc);
    if constexpr (!ROWWISE) m[i] = acc;
  }
  tbl_st4<DT>(W, widx, w, stream);
  double part = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) part += (double)w[i] * (double)w[i] - (double)w0[i] * (double)w0[i];
  return part;
}

// 16 category rows, one per 16-lane group (update_cate_rows_opt's walk)
template <int NC, int DT, bool ROWWISE>
__device__ __forceinline__ double update_cate_rows_adagrad(const ApplyArgs& a, const AdagradCtx& x, int c, int lane,
                                                           uint32_t salt) {
  const int l16 = lane & 15;
  const bool vc = c < a.C;
  const size_t wrow = (size_t)(vc ? c : 0) * a.dc;
  f32x4 w[NC], g[NC], m[NC];
  float acc_row = 0.0f;
  // (the same for the 16 lanes of the row: a row the index counts as used has its W and accumulator requested beside its sum)
  const bool counted = vc && a.off_uc[c + 1] > a.off_uc[c];
  bool nz = counted;
  if (ROWWISE && counted) acc_row = a.s1.cate_emb[c];   // (one float of slot per row: the group's lanes ask for the same word)
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
    const size_t e = wrow + 4 * (l16 + 16 * ch);
    if (vc && 4 * (l16 + 16 * ch) < a.dc) {
      if (counted) {
        w[ch] = tbl_ld4<DT>(a.p.cate_emb, e);
        if constexpr (!ROWWISE) m[ch] = *(const f32x4*)(a.s1.cate_emb + e);
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
    if (ROWWISE && !counted) acc_row = a.s1.cate_emb[c];
    float ss = 0.0f;
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {   // (the rows reached through their items only: W and accumulator once the sum is known)
      const size_t e = wrow + 4 * (l16 + 16 * ch);
      if (4 * (l16 + 16 * ch) < a.dc) {
        if (!counted) {
          w[ch] = tbl_ld4<DT>(a.p.cate_emb, e);
          if constexpr (!ROWWISE) m[ch] = *(const f32x4*)(a.s1.cate_emb + e);
        }
        adagrad_grad4(x, w[ch], g[ch], ss);
      }
    }
    if constexpr (ROWWISE) {
      acc_row += group16_sum(ss) * (1.0f / (float)a.dc);
      if (l16 == 0) a.s1.cate_emb[c] = acc_row;
    }
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      const size_t e = wrow + 4 * (l16 + 16 * ch);
      if (4 * (l16 + 16 * ch) < a.dc) {
        part += adagrad_row4<DT, ROWWISE>(x, a.p.cate_emb, e, w[ch], g[ch], m[ch], acc_row, salt ^ 0x3c6ef372u);
        if constexpr (!ROWWISE) *(f32x4*)(a.s1.cate_emb + e) = m[ch];
      }
    }
  }
  return part;
}

// grid: nbC16 = ceil(C / 16) blocks of category rows, nbI / nbU blocks of used item / user rows
// (one row per 16-lane group), nbD blocks of 256 dense parameters
template <bool WIDE, int DT, bool ROWWISE>
__global__ __launch_bounds__(256) void k_update_lazy_adagrad(ApplyArgs a, int nbC16) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  __shared__ double shp[4];
  const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, gid = tid >> 4, blk = blockIdx.x;
  AdagradCtx x;
  x.lr = a.lr;
  x.coef = a.hdr->coef;
  x.reg = a.reg;
  x.P = a.hdr->P;   // (not committed by this step's finalize)
  x.invP = 1.0f / x.P;
  const uint32_t salt = a.hdr->nstep;
  if (blk == 0 && tid == 0) a.hdr->spart_n[salt & 1] = nbC16 + a.nbI + a.nbU;
  double part = 0.0;
  if (blk < nbC16) {
    part = update_cate_rows_adagrad<NC, DT, ROWWISE>(a, x, blk * 16 + gid, lane, salt);
  } else if (blk < nbC16 + a.nbI) {
    const int slot0 = (blk - nbC16) * AP_ROWS_PB, slot = slot0 + gid;
    const int nuq = *a.n_uniq_item;
    if (slot0 >= nuq) return;
    if (slot < nuq) {
      const int row = a.urec_item[slot].x;
      const size_t wrow = (size_t)row * a.p.ld_item;
      float* S1 = ROWWISE ? a.s1.item_emb + row : a.s1.item_emb + (size_t)row * a.s1.ld_item;   // the row's float | its row of floats
      f32x4 w[NI], g[NI], m[NI];
      float wb = 0.0f, gb = 0.0f, acc_row = 0.0f;
      if constexpr (ROWWISE) acc_row = *S1;
#pragma unroll
      for (int ch = 0; ch < NI; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          w[ch] = tbl_ld4<DT>(a.p.item_emb, wrow + cc);
          g[ch] = *(const f32x4*)(a.Ri + (size_t)slot * a.di + cc);
          if constexpr (!ROWWISE) m[ch] = *(const f32x4*)(S1 + cc);
        }
      }
      if (l16 == 0) { wb = a.p.item_b[(size_t)row * a.p.ld_itemb]; gb = a.Rb[slot]; }
      float ss = 0.0f;   // (lanes and chunks past the row's width add nothing: exactly 0)
#pragma unroll
      for (int ch = 0; ch < NI; ++ch)
        if (4 * (l16 + 16 * ch) < a.di) adagrad_grad4(x, w[ch], g[ch], ss);
      if constexpr (ROWWISE) {
        acc_row += group16_sum(ss) * (1.0f / (float)a.di);
        if (l16 == 0) *S1 = acc_row;
      }
#pragma unroll
      for (int ch = 0; ch < NI; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          part += adagrad_row4<DT, ROWWISE>(x, a.p.item_emb, wrow + cc, w[ch], g[ch], m[ch], acc_row, salt ^ 0x85ebca6bu);
          if constexpr (!ROWWISE) *(f32x4*)(S1 + cc) = m[ch];
        }
      }
      if (l16 == 0 && gb != 0.0f) {   // item_b: not regularised; moves where the candidates gave it a gradient (k_apply)
        float* q1 = a.s1.item_b + (size_t)row * a.s1.ld_itemb;
        float a1 = *q1;
        a.p.item_b[(size_t)row * a.p.ld_itemb] = adagrad_elem(x.lr, wb, x.coef * gb, a1);
        *q1 = a1;
      }
    }
  } else if (blk < nbC16 + a.nbI + a.nbU) {
    const int slot0 = (blk - nbC16 - a.nbI) * AP_ROWS_PB, slot = slot0 + gid;
    const int nuq = *a.n_uniq_user;
    if (slot0 >= nuq) return;
    if (slot < nuq) {
      const int row = a.urec_user[slot].x;
      const size_t wrow = (size_t)row * a.p.ld_user;
      float* S1 = ROWWISE ? a.s1.user_emb + row : a.s1.user_emb + (size_t)row * a.s1.ld_user;
      float* Trow = a.p.usert_emb + (size_t)row * a.p.ld_usert;
      float* T1 = ROWWISE ? a.s1.usert_emb + row : a.s1.usert_emb + (size_t)row * a.s1.ld_usert;
      f32x4 w[NU], g[NU], m[NU];
      float acc_u = 0.0f, acc_t = 0.0f;   // row-wise: user_emb and usert_emb are two variables, an accumulator each
      if constexpr (ROWWISE) { acc_u = *S1; acc_t = *T1; }
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.WU) g[ch] = *(const f32x4*)(a.Ru + (size_t)slot * a.WU + cc);
        if (cc < a.di) {
          w[ch] = tbl_ld4<DT>(a.p.user_emb, wrow + cc);
          if constexpr (!ROWWISE) m[ch] = *(const f32x4*)(S1 + cc);
        } else if (cc < a.WU) {   // usert_emb columns (scalar: Ls need not be a multiple of 4)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int p = cc + i - a.di;
            const bool in = p < a.Ls;
            w[ch][i] = in ? Trow[p] : 0.0f;
            if constexpr (!ROWWISE) m[ch][i] = in ? T1[p] : 0.0f;
          }
        }
      }
      float ss_u = 0.0f, ss_t = 0.0f;   // the two variables' columns form their own sums
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          adagrad_grad4(x, w[ch], g[ch], ss_u);
        } else if (cc < a.WU) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cc + i - a.di < a.Ls) {   // (the padding columns of the sum's row are not the variable's)
              const float gi = x.coef * (g[ch][i] + x.reg * (x.P * w[ch][i]));
              g[ch][i] = gi;
              ss_t += gi * gi;
            }
        }
      }
      if constexpr (ROWWISE) {
        acc_u += group16_sum(ss_u) * (1.0f / (float)a.di);
        acc_t += group16_sum(ss_t) * (1.0f / (float)a.Ls);
        if (l16 == 0) { *S1 = acc_u; *T1 = acc_t; }
      }
#pragma unroll
      for (int ch = 0; ch < NU; ++ch) {
        const int cc = 4 * (l16 + 16 * ch);
        if (cc < a.di) {
          part += adagrad_row4<DT, ROWWISE>(x, a.p.user_emb, wrow + cc, w[ch], g[ch], m[ch], acc_u, salt ^ 0xc2b2ae35u);
          if constexpr (!ROWWISE) *(f32x4*)(S1 + cc) = m[ch];
        } else if (cc < a.WU) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int p = cc + i - a.di;
            if (p < a.Ls) {
              const float w0 = w[ch][i];
              float acc = ROWWISE ? acc_t : m[ch][i];
              const float wn = adagrad_scaled<ROWWISE>(x, w0, g[ch][i], acc);
              Trow[p] = wn;
              if constexpr (!ROWWISE) T1[p] = acc;
              part += (double)wn * (double)wn - (double)w0 * (double)w0;
            }
          }
        }
      }
    }
  } else {
    const int nd = (blk - nbC16 - a.nbI - a.nbU) * 256 + tid;
    if (nd < a.lay.n_dense) {
      float a1 = a.s1.dense[nd];
      const float wn = adagrad_elem(x.lr, a.p.dense[nd], x.coef * a.gd[nd], a1);
      a.s1.dense[nd] = a1;
      dense_store(a, nd, wn);
    }
    return;
  }
  block_delta_store(part, shp, a, blk, salt);
}

// tlsan_fix.h -- the correcting pass of a clipped speculative step, shared by k_spec_commit (three launches), the head
// of the next k_fwd_bwd (spec_fix_head, tlsan_attn.h) and k_spec_flush (two launches).  A unit whose workgroups are larger
// than 256 threads defines AP_SYNC() before it includes this header (tlsan_apply.h).
#pragma once
#include "tlsan_apply.h"

struct FixLds { double* shd; double* shp; int* sh_pos; int* sh_lo; int* sh_n; int* sh_wtot; };   // the row block functions' scratch
// ... and its size, for a caller that carves it from a block of its own (spec_fix_head, tlsan_attn.h): shd as the wide form
// wants it (two float4 chunks per lane), then shp[4], sh_pos[AP_CAP], sh_lo[256], sh_n[256], sh_wtot[4]
constexpr int FIX_SHD_DOUBLES = 4 * 16 * 2 * 4;
constexpr int FIX_LDS_BYTES = 8 * FIX_SHD_DOUBLES + 8 * 4 + 4 * AP_CAP + 4 * 256 + 4 * 256 + 4 * 4;

// rows: w_spec + (scale_spec - scale_true) * sum, i.e. w_old - scale_true * sum up to one rounding; the scalars are the
// clipped step's, as its summary left them (P_prev, spec_salt, coef)
__device__ __forceinline__ ApCtx spec_fix_ctx(const ApplyArgs& a) {
  const int tid = threadIdx.x;
  const float st_true = a.lr * a.hdr->coef;
  ApCtx x;
  x.tid = tid; x.wave = tid >> 6; x.lane = tid & 63; x.grp = x.lane >> 4; x.l16 = x.lane & 15;
  x.gid = x.wave * 4 + x.grp;
  x.blk = 0;
  x.P = a.hdr->P_prev;
  x.invP = 1.0f / x.P;
  x.step = st_true - a.lr;                                                   // item_b: w_spec - (st_true - lr) g = w_old - st_true g
  x.lazy_scale = st_true / (x.P * (1.0f - st_true * a.reg)) - a.lr / (x.P * (1.0f - a.lr * a.reg));
  x.salt = a.hdr->spec_salt;
  x.coef = a.hdr->coef;
  x.accum = true;
  return x;
}

// 256 threads take the row blocks v0, v0 + stride, ... of [hot rows | categories | item rows | user rows] (not for shared
// categories) and, with `dense`, the blocks of 256 dense parameters the same way (the two-launch form stored them with
// coefficient 1 as well: dense_finalize_block)
template <bool WIDE, int DT>
__device__ __forceinline__ void spec_fix_blocks(const ApplyArgs& a, ApCtx& x, int v0, int stride, bool dense, const FixLds& m) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  constexpr int OWN = WIDE ? SPEC_OWN : AP_OWN;
  for (int v = v0; v < a.nbH + a.nbC + a.nbI + a.nbU; v += stride) {
    if (v < a.nbH) {
      presum_hot_block<NI, true, DT>(a, v, m.shd, m.shp, &x);
    } else {
      const int blk = v - a.nbH;
      x.blk = blk;
      if (blk < a.nbC) {
        if (WIDE || a.cseg) apply_cseg_block<AP_UPDATE, true, NC, OWN, DT>(a, x, blk * AP_ROWS_PB, m.shp);
        else apply_cate_block<AP_UPDATE, true, NC, DT>(a, x, m.shd, m.shp, m.sh_pos, m.sh_lo, m.sh_n, m.sh_wtot);
      }
      else if (blk < a.nbC + a.nbI) apply_rows_block<AP_UPDATE, true, true, NI, OWN, DT>(a, x, (blk - a.nbC) * AP_ROWS_PB, m.shp);
      else apply_rows_block<AP_UPDATE, true, false, NU, (WIDE ? SPEC_OWN : AP_OWN / 2), DT>(a, x, (blk - a.nbC - a.nbI) * AP_ROWS_PB, m.shp);
    }
    AP_SYNC();   // (the shared scratch is reused by the next block of rows)
  }
  if (dense) {
    for (int v = v0; v < a.nbD; v += stride) {
      const int nd = v * 256 + x.tid;
      if (nd < a.lay.n_dense) dense_store(a, nd, a.p.dense[nd] - x.step * a.gd[nd]);
    }
  }
}


// tlsan_apply.h -- the row updates: exact sum of every destination row's contiguous segment(s) of per-use gradient rows
// + clip + SGD or optimizer step (model.py:198-205), as block functions that a workgroup of 256 threads runs
// (apply_cate_block, apply_rows_block, apply_cseg_block, presum_hot_block) and the one launch that applies them to all
// tables (k_apply); also run by the finalize launches with row workgroups (tlsan_finalize_rows.h) and the correcting pass
// (tlsan_fix.h).  Determinism: the float sums are order-independent (exact_term) or in a fixed order.
#pragma once
#include "tlsan_update_args.h"
#include "tlsan_opt.h"

// exact sum of rows lo, lo+stride, ... < hi of a [.., ld] buffer (columns 4*c4..), 4 in flight
template <int NCH>
__device__ __forceinline__ void seg_accum(const float* __restrict__ Gs, int ld, int lo, int hi, int stride,
                                          int W4, int l16, double (&acc)[NCH][4]) {
  for (int k = lo; k < hi; k += 4 * stride) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c4 = l16 + 16 * ch;
      if (c4 < W4) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          v[u] = (k + u * stride < hi) ? *(const f32x4*)(Gs + (size_t)(k + u * stride) * ld + 4 * c4) : (f32x4)(0.0f);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[ch][i] += exact_term(v[u][i]);
      }
    }
  }
}

template <int NCH>
__device__ __forceinline__ void zero_acc(double (&acc)[NCH][4]) {
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[ch][i] = 0.0;
}

// sum over the four 16-lane groups of a wavefront (exact doubles -> order irrelevant)
template <int NCH>
__device__ __forceinline__ void combine_groups(double (&acc)[NCH][4]) {
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[ch][i] += __shfl_xor(acc[ch][i], 16);
      acc[ch][i] += __shfl_xor(acc[ch][i], 32);
    }
}

// The barrier of the 256 threads that run a row block function.  A unit whose workgroups are larger (the fused kernel,
// whose first four wavefronts run the correcting pass of a clipped two-launch step: spec_fix_head, tlsan_attn.h) defines
// its own before it includes this header.
#ifndef AP_SYNC
#define AP_SYNC() __syncthreads()
#endif

// record i of step `tag` (in that step's parity array of a.delta_out).  accum: add to the record this step's first launch
// left (the correcting pass of a speculative update, k_spec_commit)
__device__ __forceinline__ void block_delta_store(double part, double* shd, const ApplyArgs& a, int i, unsigned long long tag, bool accum = false) {
  AP_SYNC();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) part += __shfl_xor(part, o);
  if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = part;
  AP_SYNC();
  if (threadIdx.x == 0) {
    DeltaRec* dst = delta_recs(a.delta_out, a.delta_nrec, tag) + i;
    const double v = shd[0] + shd[1] + shd[2] + shd[3];
    dst->v = (accum && dst->tag == tag) ? dst->v + v : v;
    dst->tag = tag;
  }
}

__device__ __forceinline__ void block_part_store(double part, double* shd, double* dst) {
  __syncthreads();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) part += __shfl_xor(part, o);
  if ((threadIdx.x & 63) == 0) shd[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) *dst = shd[0] + shd[1] + shd[2] + shd[3];
}

// One parameter element of a regularised table under the update of model.py:198-205.
// Stored value w (true parameter P*w), exact gradient sum gs of the TRUE parameter.
//   dense : w <- w - step * (gs / P + reg * w)            (every row, every step)
//   lazy  : w <- w - (step / P_new) * gs, P_new = P (1 - step reg), P committed once per step
// Returns the gradient (GRADS / ROWNORM) and accumulates the block partial.
template <int MODE, bool LAZY>
__device__ __forceinline__ float apply_elem(float& w, float gs, float P, float invP, float reg, float step,
                                            float lazy_scale, double& part) {
  const float g = gs + reg * (P * w);  // gradient of the true parameter
  if constexpr (MODE == AP_SUMSQ) part += (double)w * (double)w;
  if constexpr (MODE == AP_ROWNORM) part += (double)g * (double)g;
  if constexpr (MODE == AP_UPDATE) {
    const float w0 = w;
    if constexpr (LAZY) w = w0 - lazy_scale * gs;
    else w = w0 - step * (gs * invP + reg * w0);
    part += (double)w * (double)w - (double)w0 * (double)w0;
  }
  return g;
}

// ------------------------------------------------------------------------------------------
// k_apply: ONE launch applies the step to every embedding table and the dense parameters.
// Block layout: [0,nbC) one category row per workgroup, then nbI blocks of item rows and nbU
// blocks of user rows (user_emb + usert_emb; one row per 16-lane group), then nbD blocks of 256
// dense parameters.  Category blocks come first: they have the longest dependent chain.
//
// Item uses are stored destination-sorted as rows [item half | cate half] of Gi: the item
// blocks sum the item halves of their row's contiguous segment, the category blocks sum the
// cate halves of the segments of all items of the category (static CSR of item_cate) plus the
// category's u_cate uses (segment of Gc).  Nothing is passed between blocks, so rows and
// categories need no second launch.  Every sum is exact (exact_term) -> order-free, bitwise
// reproducible.
//
// The kernel is a chain of dependent memory round trips, so every load that does not depend
// on another is issued up front: used-row records, clip-norm partials, the parameter row, and
// the first AP_OWN gradient rows of a segment in one batch (clamped addresses instead of
// branches, which the compiler would serialise).
// LAZY (apply_*_block): the row blocks walk the compacted records of used rows (k_index_scan) instead of every row.
// NCH = float4 chunks per lane: 16 lanes x NCH x 4 floats >= the widest row (d_item, WU, d_cate).
#define AP_CAP 2048  // LDS list of use positions of one category pass

// exact sum of the rows listed in sh_pos[0, T): >= 0 -> cate half of Gi[pos], < 0 -> Gc[~pos];
// the 16 groups of the workgroup stride over the list, AP_OWN rows in flight per group
template <int NCH>
__device__ __forceinline__ void list_accum(const ApplyArgs& a, const int* sh_pos, int T, int gid, int l16, int W4,
                                           double (&acc)[NCH][4]) {
  for (int k = gid; k < T; k += 16 * AP_OWN) {
    f32x4 v[AP_OWN][NCH];
#pragma unroll
    for (int u = 0; u < AP_OWN; ++u) {
      const int kk = k + 16 * u;
      const int pos = sh_pos[kk < T ? kk : k];
      const float* src = pos >= 0 ? a.Gi + (size_t)pos * a.D + a.di : a.Gc + (size_t)(~pos) * a.dc;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c4 = l16 + 16 * ch;
        if (c4 < W4) v[u][ch] = *(const f32x4*)(src + 4 * c4);
      }
    }
#pragma unroll
    for (int u = 0; u < AP_OWN; ++u) {
      if (k + 16 * u < T) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          if (l16 + 16 * ch < W4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[ch][i] += exact_term(v[u][ch][i]);
          }
        }
      }
    }
  }
}

struct ApCtx {
  int tid, wave, lane, grp, l16, gid, blk;
  float P, invP, step, lazy_scale;
  uint32_t salt;      // per-step salt of the stochastic rounding (bf16 tables)
  float coef;         // clip coefficient (optimizers other than SGD)
  OptCtx oc;
  bool accum = false; // UPDATE: add the block's change of the sum of squares to its record of this step (k_spec_commit)
};

// A row workgroup's context: its lanes' roles, its record (blk0: the workgroups that lead the grid) and the step's scalars
// (lazy_scale: the lazy-L2 step's scale of the exact sum, apply_elem)
__device__ __forceinline__ ApCtx ap_ctx(const ApplyArgs& a, int blk0, float P, float step, uint32_t salt, float coef) {
  ApCtx x;
  x.tid = threadIdx.x; x.wave = x.tid >> 6; x.lane = x.tid & 63; x.grp = x.lane >> 4; x.l16 = x.lane & 15;
  x.gid = x.wave * 4 + x.grp;  // 16 groups
  x.blk = blockIdx.x - blk0;
  x.P = P;
  x.invP = 1.0f / P;
  x.step = step;
  x.lazy_scale = step / (P * (1.0f - step * a.reg));
  x.salt = salt;
  x.coef = coef;
  x.oc.opt = a.opt; x.oc.lr = a.lr; x.oc.b1 = a.ob1; x.oc.b2 = a.ob2; x.oc.eps = a.oeps; x.oc.alpha = a.oalpha;
  return x;
}

#define AP_STAMP(k)                                                                      \
  do {                                                                                   \
    if (a.stamps != nullptr && x.tid == 0) a.stamps[(size_t)x.blk * 8 + (k)] = __builtin_amdgcn_s_memtime(); \
  } while (0)

// A dense parameter's new value, and its copy in dense_KT (K transposed) when it is one of K's
__device__ __forceinline__ void dense_store(const ApplyArgs& a, int nd, float wn) {
  a.p.dense[nd] = wn;
  if (nd >= a.lay.K && nd < a.lay.k0) {
    const int idx = nd - a.lay.K;
    a.p.dense_KT[(size_t)(idx % a.D) * a.D + idx / a.D] = wn;
  }
}

// ================= one category row per workgroup =================
template <int MODE, bool LAZY, int NCH, int DT, bool CSPLIT = false>
__device__ __forceinline__ void apply_cate_block(const ApplyArgs& a, const ApCtx& x, double* shd, double* shp,
                                                 int* sh_pos, int* sh_lo, int* sh_n, int* sh_wtot) {
  constexpr bool RESET = MODE == AP_UPDATE || MODE == AP_GRADS || MODE == AP_PRESUM;  // counters are zero at rest
  const int tid = x.tid, wave = x.wave, lane = x.lane, grp = x.grp, l16 = x.l16, gid = x.gid;
  int c = x.blk, split = 0, nsplit = 1;
  if constexpr (MODE == AP_PRESUM && CSPLIT) {  // (a compile-time variant: the common single-workgroup case pays nothing)
    nsplit = a.csplit; c = x.blk % a.C; split = x.blk / a.C;
  }
  const int W4 = a.dc / 4;
  const size_t wrow = (size_t)c * a.dc;  // element index of the row in cate_emb
  f32x4 w[NCH];
  if constexpr (MODE != AP_PRESUM) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
      if (l16 + 16 * ch < W4) w[ch] = tbl_ld4<DT>(a.p.cate_emb, wrow + 4 * (l16 + 16 * ch));
  }
  double acc[NCH][4];
  zero_acc(acc);
  double part = 0.0;
  int nu = 0;
  if constexpr (MODE != AP_SUMSQ) {
    // (CSEG: nothing to walk -- the category halves of the items' uses sit in this category's segment of Gc, with the
    //  u_cate uses: `nu` below counts both)
    const int i0 = a.cseg ? 0 : a.cate_off[c], ni = a.cseg ? 0 : a.cate_cnt[c];
    int ou = a.off_uc[c];
    const int nu_all = a.off_uc[c + 1] - ou;
    nu = nu_all;
    int PS = 256;  // items per pass
    bool by_pos = false;     // (CSPLIT) shares are slices of the use positions, not groups of items
    if constexpr (CSPLIT) {  // this workgroup's share of the u_cate uses and its pass size
      by_pos = a.cpos != 0;
      if (!by_pos) PS = a.cpass;
      const int chunk = (nu_all + nsplit - 1) / nsplit;
      ou += split * chunk;
      nu = max(0, min(chunk, nu_all - split * chunk));
    }
    const int pstart = by_pos ? 0 : split * PS, pstep = by_pos ? PS : nsplit * PS;
    bool first = true;
    for (int p0 = pstart; first || p0 < ni; p0 += pstep, first = false) {
      int lo = 0, n = 0;
      if (tid < PS && p0 + tid < ni) {
        const int item = a.cate_items[i0 + p0 + tid];
        lo = a.off_item[item];
        n = a.off_item[item + 1] - lo;
      }
      int inc = n;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
      }
      if (lane == 63) sh_wtot[wave] = inc;
      AP_SYNC();
      int pre = inc - n;
#pragma unroll
      for (int w_ = 0; w_ < 4; ++w_) pre += (w_ < wave) ? sh_wtot[w_] : 0;
      int T = (sh_wtot[0] + sh_wtot[1]) + (sh_wtot[2] + sh_wtot[3]);
      const bool last = p0 + pstep >= ni;  // this workgroup's last pass
      const int extra = last ? nu : 0;  // the u_cate uses ride along with the last pass
      // by_pos: this workgroup's slice [s_lo, s_hi) of the pass's T concatenated use positions
      int s_lo = 0, s_hi = T;
      if (by_pos) {
        s_lo = (int)((long long)T * split / nsplit);
        s_hi = (int)((long long)T * (split + 1) / nsplit);
        T = s_hi - s_lo;
      }
      if (T + extra <= AP_CAP) {
        if constexpr (CSPLIT) {
          for (int j = max(0, s_lo - pre); j < min(n, s_hi - pre); ++j) sh_pos[pre + j - s_lo] = lo + j;
        } else {   // (the whole pass: no slice arithmetic in the registers of the one-workgroup-per-category form)
          for (int j = 0; j < n; ++j) sh_pos[pre + j] = lo + j;
        }
        for (int j = tid; j < extra; j += 256) sh_pos[T + j] = ~(a.uc_list ? a.uc_list[ou + j] : ou + j);
        AP_SYNC();
        AP_STAMP(1);
        list_accum<NCH>(a, sh_pos, T + extra, gid, l16, W4, acc);
        AP_STAMP(2);
      } else {  // very hot category: segment after segment, the 16 groups striding over each
        sh_lo[tid] = lo;
        sh_n[tid] = n;
        AP_SYNC();
        const int cnt = max(0, min(PS, ni - p0));
        int run = 0;   // (by_pos) concatenated position of the segment's first use
        for (int t = 0; t < cnt; ++t) {
          const int nt = sh_n[t], lt = sh_lo[t];
          if constexpr (CSPLIT) {
            const int o_lo = max(run, s_lo), o_hi = min(run + nt, s_hi);   // the part of the segment inside the slice
            if (o_hi > o_lo) seg_accum<NCH>(a.Gi + a.di, a.D, lt + (o_lo - run) + gid, lt + (o_hi - run), 16, W4, l16, acc);
            run += nt;
          } else {
            if (nt > 0) seg_accum<NCH>(a.Gi + a.di, a.D, lt + gid, lt + nt, 16, W4, l16, acc);
          }
        }
        if (last) {
          if (a.uc_list == nullptr) {
            seg_accum<NCH>(a.Gc, a.dc, ou + gid, ou + nu, 16, W4, l16, acc);
          } else {  // (rows in sample order: through the category's sample list)
            for (int k = ou + gid; k < ou + nu; k += 16) {
              const float* src = a.Gc + (size_t)a.uc_list[k] * a.dc;
#pragma unroll
              for (int ch = 0; ch < NCH; ++ch)
                if (l16 + 16 * ch < W4) {
                  const f32x4 v = *(const f32x4*)(src + 4 * (l16 + 16 * ch));
#pragma unroll
                  for (int i = 0; i < 4; ++i) acc[ch][i] += exact_term(v[i]);
                }
            }
          }
        }
      }
      AP_SYNC();  // sh_pos / sh_wtot are rewritten by the next pass
    }
    combine_groups(acc);
    if (grp == 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) shd[((wave * 16 + l16) * NCH + ch) * 4 + i] = acc[ch][i];
    }
    AP_SYNC();
    if (wave == 0 && grp == 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double s = 0.0;
          for (int w_ = 0; w_ < 4; ++w_) s += shd[((w_ * 16 + l16) * NCH + ch) * 4 + i];
          acc[ch][i] = s;
        }
    }
  }
  AP_STAMP(3);
  if constexpr (MODE == AP_PRESUM) {
    if (wave == 0 && grp == 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c4 = l16 + 16 * ch;
        if (c4 < W4) {
          if constexpr (CSPLIT) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (acc[ch][i] != 0.0) unsafeAtomicAdd(a.Rc64 + wrow + 4 * c4 + i, acc[ch][i]);  // (hardware f64 add, no CAS loop)
          } else {
            f32x4 g;
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = (float)acc[ch][i];
            *(f32x4*)(a.Rc + wrow + 4 * c4) = g;
          }
        }
      }
    }
    if (tid == 0 && split == 0 && nu > 0) a.cnt_uc[c] = 0;
    return;
  }
  if (wave == 0 && grp == 0) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c4 = l16 + 16 * ch;
      if (c4 < W4) {
        f32x4 g;
        const f32x4 w0 = w[ch];
        double pe = 0.0;  // (UPDATE: the change of the sum of squares is taken from the values actually stored)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float wi = w[ch][i];
          g[i] = apply_elem<MODE, LAZY>(wi, (float)acc[ch][i], x.P, x.invP, a.reg, x.step, x.lazy_scale, pe);
          w[ch][i] = wi;
        }
        if constexpr (MODE == AP_GRADS) *(f32x4*)(a.go.cate_emb + (size_t)c * a.dc + 4 * c4) = g;
        if constexpr (MODE == AP_UPDATE && !LAZY) {
          if (a.opt != TLSAN_OPT_SGD) {
            f32x4 m1 = *(const f32x4*)(a.s1.cate_emb + wrow + 4 * c4), m2 = *(const f32x4*)(a.s2.cate_emb + wrow + 4 * c4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float wi = w0[i], a1 = m1[i], a2 = m2[i];
              opt_elem(x.oc, wi, x.coef * g[i], a1, a2);
              w[ch][i] = wi; m1[i] = a1; m2[i] = a2;
            }
            *(f32x4*)(a.s1.cate_emb + wrow + 4 * c4) = m1;
            *(f32x4*)(a.s2.cate_emb + wrow + 4 * c4) = m2;
          }
        }
        if constexpr (MODE == AP_UPDATE) {
          tbl_st4<DT>(a.p.cate_emb, wrow + 4 * c4, w[ch], x.salt ^ 0x3c6ef372u);
#pragma unroll
          for (int i = 0; i < 4; ++i) part += (double)w[ch][i] * (double)w[ch][i] - (double)w0[i] * (double)w0[i];
        } else {
          part += pe;
        }
      }
    }
  }
  if constexpr (RESET) {
    if (tid == 0 && nu > 0) a.cnt_uc[c] = 0;
  }
  if constexpr (MODE == AP_UPDATE) block_delta_store(part, shp, a, x.blk, x.salt, x.accum);
  else if constexpr (MODE != AP_GRADS) block_part_store(part, shp, &a.part_out[x.blk]);
}

// ================= 16 item rows or 16 user rows per workgroup (one row per 16-lane group) =========
// NCH float4 chunks per lane cover the row (item rows: the item half only), OWN gradient rows are
// in flight per group; longer segments are finished by the whole wavefront.
// C0: first 16-byte chunk per lane this call covers (a row wider than 16 lanes x NCH chunks is covered by two calls:
// the row sums of 154-float user rows -- d = 128 with 90-entry windows -- without the wide variant's registers)
template <int MODE, bool LAZY, bool IS_ITEM, int NCH, int OWN, int DT, int C0 = 0>
__device__ __forceinline__ void apply_rows_block(const ApplyArgs& a, const ApCtx& x, int slot0, double* shp) {
  constexpr bool RESET = MODE == AP_UPDATE || MODE == AP_GRADS || MODE == AP_PRESUM;
  const int lane = x.lane, grp = x.grp, l16 = x.l16;
  const int slot = slot0 + x.gid;
  int row = 0, off = 0, n = 0;
  bool vr;
  double part = 0.0;
  if constexpr (LAZY) {
    const int nuq = IS_ITEM ? *a.n_uniq_item : *a.n_uniq_user;
    if (slot0 >= nuq) return;  // (workgroup-uniform) nothing left: lazy rows past the used ones leave no partial
    const int4 r = (IS_ITEM ? a.urec_item : a.urec_user)[slot];  // (row, first position, uses)
    vr = slot < nuq;
    if (vr) { row = r.x; off = r.y; n = r.z; }
    if constexpr ((MODE == AP_PRESUM || MODE == AP_UPDATE) && IS_ITEM) {
      if (a.nbH > 0 && n > AP_HOT && *a.hot_n <= AP_HOT_CAP) { vr = false; n = 0; }   // a hot-row workgroup sums (speculative one-pass update: updates) it
    }
  } else {
    vr = slot < (IS_ITEM ? a.I : a.U);
    if (vr) row = slot;
    if constexpr (MODE != AP_SUMSQ) {
      const int32_t* o = IS_ITEM ? a.off_item : a.off_user;
      off = o[row];
      n = vr ? o[row + 1] - off : 0;
    }
  }
  AP_STAMP(1);
  const float* Gs = IS_ITEM ? a.Gi : a.Gu;
  const int ld = IS_ITEM ? a.D : a.WU;
  const int W4 = (IS_ITEM ? a.di : a.WU) / 4;
  // ---- the parameter row
  float* Wtab = IS_ITEM ? a.p.item_emb : a.p.user_emb;
  const size_t wrow = IS_ITEM ? (size_t)row * a.p.ld_item : (size_t)row * a.p.ld_user;  // element index of the row
  float* Trow = a.p.usert_emb + (size_t)row * a.p.ld_usert;
  f32x4 w[NCH];
  float wb = 0.0f;
  if constexpr (MODE != AP_PRESUM) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int cc = 4 * (l16 + 16 * (ch + C0));
      if (cc < a.di) {
        w[ch] = tbl_ld4<DT>(Wtab, wrow + cc);
      } else if (!IS_ITEM) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[ch][i] = (cc + i - a.di < a.Ls) ? Trow[cc + i - a.di] : 0.0f;
      }
    }
    if (IS_ITEM && l16 == 0) wb = a.p.item_b[(size_t)row * a.p.ld_itemb];
  }
  // ---- exact sum of the row's segment
  double acc[NCH][4];
  zero_acc(acc);
  double bacc = 0.0;  // item_b gradient of the row (item rows)
  if constexpr (MODE != AP_SUMSQ) {
    const int n_own = min(n, OWN);
    {
      f32x4 v[OWN][NCH];
      const int last = max(n_own - 1, 0);
#pragma unroll
      for (int u = 0; u < OWN; ++u) {
        const float* src = Gs + (size_t)(off + min(u, last)) * ld;  // (buffers carry a pad row)
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          if (l16 + 16 * (ch + C0) < W4) v[u][ch] = *(const f32x4*)(src + 4 * (l16 + 16 * (ch + C0)));
      }
      float gb = 0.0f;
      if (IS_ITEM) gb = a.Gb[off + min(l16, last)];
#pragma unroll
      for (int u = 0; u < OWN; ++u) {
        if (u < n_own) {
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
            if (l16 + 16 * (ch + C0) < W4) {
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[ch][i] += exact_term(v[u][ch][i]);
            }
        }
      }
      if (IS_ITEM && l16 < n_own) bacc = exact_term(gb);
    }
    AP_STAMP(2);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ng = __shfl(n, g * 16);
      if (ng > OWN) {  // wave-uniform: the four groups split the rest of group g's segment
        const int og = __shfl(off, g * 16);
        double t[NCH][4];
        zero_acc(t);
        seg_accum<NCH>(Gs + 64 * C0, ld, og + OWN + grp, og + ng, 4, W4 - 16 * C0, l16, t);
        double tb = 0.0;
        if (IS_ITEM)
          for (int k = og + OWN + lane; k < og + ng; k += 64) tb += exact_term(a.Gb[k]);
        combine_groups(t);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) tb += __shfl_xor(tb, o);
        if (grp == g) {
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[ch][i] += t[ch][i];
          if (l16 == 0) bacc += tb;
        }
      }
    }
    if (IS_ITEM) {  // fold the group's 16 partial bias sums (exact doubles: any order)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) bacc += __shfl_xor(bacc, o);
    }
  }
  AP_STAMP(3);
  if constexpr (MODE == AP_PRESUM) {
    if (vr) {
      const bool by_row = a.presum_rows != 0;  // (workgroup-uniform)
      float* R = IS_ITEM ? a.Ri + (size_t)slot * a.di : a.Ru + (size_t)slot * a.WU;
      if (by_row) R = IS_ITEM ? a.go.item_emb + (size_t)row * a.go.ld_item : a.go.user_emb + (size_t)row * a.go.ld_user;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c4 = l16 + 16 * (ch + C0);
        if (c4 < W4) {
          f32x4 g;
#pragma unroll
          for (int i = 0; i < 4; ++i) g[i] = (float)acc[ch][i];
          if (!by_row || 4 * c4 < a.di) {
            *(f32x4*)(R + 4 * c4) = g;
          } else {  // usert_emb columns of a user row
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int p = 4 * c4 + i - a.di;
              if (p < a.Ls) a.go.usert_emb[(size_t)row * a.go.ld_usert + p] = g[i];
            }
          }
        }
      }
      if (l16 == 0) {
        if (IS_ITEM) (by_row ? a.go.item_b[(size_t)row * a.go.ld_itemb] : a.Rb[slot]) = (float)bacc;
        if (n > 0) (IS_ITEM ? a.cnt_item : a.cnt_user)[row] = 0;
      }
      if (a.presum_rows == 2) {
        // fused rows [item_emb | item_b | pad] / [user_emb | usert_emb | pad] of one width (the sharded step):
        // a row is written by exactly one of the two views -- clear the rest of it, so that the caller's
        // buffer need not be zeroed
        const int first = IS_ITEM ? a.di + 1 : a.di + a.Ls, width = IS_ITEM ? a.go.ld_item : a.go.ld_user;
        for (int c = first + l16; c < width; c += 16) R[c] = 0.0f;
      }
    }
    return;
  }
  if (vr) {
    // column cc of the row: cc < di -> item_emb / user_emb;  user rows, di <= cc < di+Ls -> usert_emb
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int cc = 4 * (l16 + 16 * (ch + C0));
      if (cc >= 4 * W4) continue;
      f32x4 g;
      if (cc < a.di) {
        const f32x4 w0 = w[ch];
        double pe = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float wi = w[ch][i];
          g[i] = apply_elem<MODE, LAZY>(wi, (float)acc[ch][i], x.P, x.invP, a.reg, x.step, x.lazy_scale, pe);
          w[ch][i] = wi;
        }
        if constexpr (MODE == AP_UPDATE && !LAZY) {
          if (a.opt != TLSAN_OPT_SGD) {
            float* S1 = IS_ITEM ? a.s1.item_emb + (size_t)row * a.s1.ld_item : a.s1.user_emb + (size_t)row * a.s1.ld_user;
            float* S2 = IS_ITEM ? a.s2.item_emb + (size_t)row * a.s2.ld_item : a.s2.user_emb + (size_t)row * a.s2.ld_user;
            f32x4 m1 = *(const f32x4*)(S1 + cc), m2 = *(const f32x4*)(S2 + cc);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float wi = w0[i], a1 = m1[i], a2 = m2[i];
              opt_elem(x.oc, wi, x.coef * g[i], a1, a2);
              w[ch][i] = wi; m1[i] = a1; m2[i] = a2;
            }
            *(f32x4*)(S1 + cc) = m1;
            *(f32x4*)(S2 + cc) = m2;
          }
        }
        if constexpr (MODE == AP_GRADS) {
          if (!a.go.sparse || n > 0)
            *(f32x4*)((IS_ITEM ? a.go.item_emb + (size_t)row * a.go.ld_item : a.go.user_emb + (size_t)row * a.go.ld_user) + cc) = g;
        }
        if constexpr (MODE == AP_UPDATE) {
          tbl_st4<DT>(Wtab, wrow + cc, w[ch], x.salt ^ (IS_ITEM ? 0x85ebca6bu : 0xc2b2ae35u));
#pragma unroll
          for (int i = 0; i < 4; ++i) part += (double)w[ch][i] * (double)w[ch][i] - (double)w0[i] * (double)w0[i];
        } else {
          part += pe;
        }
      } else if (!IS_ITEM) {  // usert_emb columns (scalar: Ls need not be a multiple of 4)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = cc + i - a.di;
          if (p < a.Ls) {
            float wi = w[ch][i];
            const float w00 = wi;
            const float gg = apply_elem<MODE, LAZY>(wi, (float)acc[ch][i], x.P, x.invP, a.reg, x.step, x.lazy_scale, part);
            if constexpr (MODE == AP_GRADS) {
              if (!a.go.sparse || n > 0) a.go.usert_emb[(size_t)row * a.go.ld_usert + p] = gg;
            }
            if constexpr (MODE == AP_UPDATE && !LAZY) {
              if (a.opt != TLSAN_OPT_SGD) {
                float* q1 = a.s1.usert_emb + (size_t)row * a.s1.ld_usert + p;
                float* q2 = a.s2.usert_emb + (size_t)row * a.s2.ld_usert + p;
                float a1 = *q1, a2 = *q2;
                part -= (double)wi * (double)wi;
                wi = w00;
                opt_elem(x.oc, wi, x.coef * gg, a1, a2);
                part += (double)wi * (double)wi;
                *q1 = a1; *q2 = a2;
              }
            }
            if constexpr (MODE == AP_UPDATE) Trow[p] = wi;
          }
        }
      }
    }
    if (IS_ITEM && l16 == 0) {  // item_b[row]: not regularised (model.py:164-169), never scaled
      const float g = (float)bacc;
      if constexpr (MODE == AP_GRADS) {
        if (!a.go.sparse || n > 0) a.go.item_b[(size_t)row * a.go.ld_itemb] = g;
      }
      if constexpr (MODE == AP_ROWNORM) part += (double)g * (double)g;
      if constexpr (MODE == AP_UPDATE) {
        bool sgd = true;
        if constexpr (!LAZY) sgd = a.opt == TLSAN_OPT_SGD;
        if (sgd) {
          if (n > 0) a.p.item_b[(size_t)row * a.p.ld_itemb] = wb - x.step * g;
        } else if (g != 0.0f || a.opt == TLSAN_OPT_ADAM) {
          // sparse Adam decays m, v of every row; the sparse RMSProp / Adadelta kernels touch the rows the
          // candidates gathered -- recognised by their non-zero gradient (a candidate whose sigmoid
          // saturates to exactly y has gradient 0 and is skipped here, where TF would still decay its slots)
          float* q1 = a.s1.item_b + (size_t)row * a.s1.ld_itemb;
          float* q2 = a.s2.item_b + (size_t)row * a.s2.ld_itemb;
          float a1 = *q1, a2 = *q2, wi = wb;
          opt_elem(x.oc, wi, x.coef * g, a1, a2);
          a.p.item_b[(size_t)row * a.p.ld_itemb] = wi;
          *q1 = a1; *q2 = a2;
        }
      }
    }
    if constexpr (RESET) {
      if (n > 0 && l16 == 0) (IS_ITEM ? a.cnt_item : a.cnt_user)[row] = 0;
    }
  }
  if constexpr (MODE == AP_UPDATE) block_delta_store(part, shp, a, x.blk, x.salt, x.accum);
  else if constexpr (MODE != AP_GRADS) block_part_store(part, shp, &a.part_out[x.blk]);
}

// ================= CSEG: 16 category rows per workgroup (one per 16-lane group) =================
// With ApplyArgs.cseg a category's gradient is ONE contiguous segment of Gc (its u_cate uses and the category halves of
// its items' uses), so category rows are summed like item and user rows -- a 16-lane group per row, OWN rows in flight,
// the wavefront finishing long segments -- instead of by a workgroup each (10 k categories: 10 k workgroups of a
// few uses, each with the list machinery of apply_cate_block).  Block b handles categories [16 b, 16 b + 16).
template <int MODE, bool LAZY, int NCH, int OWN, int DT>
__device__ __forceinline__ void apply_cseg_block(const ApplyArgs& a, const ApCtx& x, int c0, double* shp) {
  constexpr bool RESET = MODE == AP_UPDATE || MODE == AP_GRADS || MODE == AP_PRESUM;
  const int lane = x.lane, grp = x.grp, l16 = x.l16;
  const int c = c0 + x.gid;
  const bool vr = c < a.C;
  const int cc = vr ? c : 0;
  const int W4 = a.dc / 4;
  int off = 0, n = 0;
  if constexpr (MODE != AP_SUMSQ) {
    off = a.off_uc[cc];
    n = vr ? a.off_uc[cc + 1] - off : 0;
  }
  const size_t wrow = (size_t)cc * a.dc;
  f32x4 w[NCH];
  if constexpr (MODE != AP_PRESUM) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
      if (l16 + 16 * ch < W4) w[ch] = tbl_ld4<DT>(a.p.cate_emb, wrow + 4 * (l16 + 16 * ch));
  }
  double acc[NCH][4];
  zero_acc(acc);
  double part = 0.0;
  if constexpr (MODE != AP_SUMSQ) {
    const int n_own = min(n, OWN);
    {
      f32x4 v[OWN][NCH];
      const int last = max(n_own - 1, 0);
#pragma unroll
      for (int u = 0; u < OWN; ++u) {
        const float* src = a.Gc + (size_t)(off + min(u, last)) * a.dc;  // (the buffer carries a pad row)
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          if (l16 + 16 * ch < W4) v[u][ch] = *(const f32x4*)(src + 4 * (l16 + 16 * ch));
      }
#pragma unroll
      for (int u = 0; u < OWN; ++u)
        if (u < n_own) {
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
            if (l16 + 16 * ch < W4) {
#pragma unroll
              for (int i = 0; i < 4; ++i) acc[ch][i] += exact_term(v[u][ch][i]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ng = __shfl(n, g * 16);
      if (ng > OWN) {  // wave-uniform: the four groups split the rest of group g's segment
        const int og = __shfl(off, g * 16);
        double t[NCH][4];
        zero_acc(t);
        seg_accum<NCH>(a.Gc, a.dc, og + OWN + grp, og + ng, 4, W4, l16, t);
        combine_groups(t);
        if (grp == g) {
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[ch][i] += t[ch][i];
        }
      }
    }
  }
  if constexpr (MODE == AP_PRESUM) {
    if (vr) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c4 = l16 + 16 * ch;
        if (c4 < W4) {
          f32x4 g;
#pragma unroll
          for (int i = 0; i < 4; ++i) g[i] = (float)acc[ch][i];
          *(f32x4*)(a.Rc + wrow + 4 * c4) = g;
        }
      }
      if (l16 == 0 && n > 0) a.cnt_uc[c] = 0;
    }
    return;
  }
  if (vr) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c4 = l16 + 16 * ch;
      if (c4 >= W4) continue;
      f32x4 g;
      const f32x4 w0 = w[ch];
      double pe = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float wi = w[ch][i];
        g[i] = apply_elem<MODE, LAZY>(wi, (float)acc[ch][i], x.P, x.invP, a.reg, x.step, x.lazy_scale, pe);
        w[ch][i] = wi;
      }
      if constexpr (MODE == AP_GRADS) *(f32x4*)(a.go.cate_emb + (size_t)c * a.dc + 4 * c4) = g;
      if constexpr (MODE == AP_UPDATE && !LAZY) {
        if (a.opt != TLSAN_OPT_SGD) {
          f32x4 m1 = *(const f32x4*)(a.s1.cate_emb + wrow + 4 * c4), m2 = *(const f32x4*)(a.s2.cate_emb + wrow + 4 * c4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float wi = w0[i], a1 = m1[i], a2 = m2[i];
            opt_elem(x.oc, wi, x.coef * g[i], a1, a2);
            w[ch][i] = wi; m1[i] = a1; m2[i] = a2;
          }
          *(f32x4*)(a.s1.cate_emb + wrow + 4 * c4) = m1;
          *(f32x4*)(a.s2.cate_emb + wrow + 4 * c4) = m2;
        }
      }
      if constexpr (MODE == AP_UPDATE) {
        tbl_st4<DT>(a.p.cate_emb, wrow + 4 * c4, w[ch], x.salt ^ 0x3c6ef372u);
#pragma unroll
        for (int i = 0; i < 4; ++i) part += (double)w[ch][i] * (double)w[ch][i] - (double)w0[i] * (double)w0[i];
      } else {
        part += pe;
      }
    }
    if constexpr (RESET) {
      if (l16 == 0 && n > 0) a.cnt_uc[c] = 0;
    }
  }
  if constexpr (MODE == AP_UPDATE) block_delta_store(part, shp, a, x.blk, x.salt, x.accum);
  else if constexpr (MODE != AP_GRADS) block_part_store(part, shp, &a.part_out[x.blk]);
}

// ================= one hot item row per workgroup (PRESUM) =================
// UPD (the speculative one-pass update, k_finalize_update / k_spec_commit): the workgroup updates the row itself --
// w -= x.lazy_scale * sum, item_b -= x.step * sum_b -- and leaves its change of the sum of squares in record
// nbC + nbI + nbU + h of S_delta (hot workgroups own the records behind the row blocks').
template <int NCH, bool UPD = false, int DT = TLSAN_TABLE_F32>
__device__ __forceinline__ void presum_hot_block(const ApplyArgs& a, int h, double* shd, double* shp, const ApCtx* xp = nullptr) {
  const int nh = *a.hot_n;
  if (nh > AP_HOT_CAP || h >= nh) return;  // (workgroup-uniform) list overflowed: the item-row workgroups kept the rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane >> 4, l16 = lane & 15, gid = wave * 4 + grp;
  const int slot = a.hot_list[h];
  const int4 r = a.urec_item[slot];
  const int row = r.x, off = r.y, n = r.z;
  const int W4 = a.di / 4;
  f32x4 w_row[NCH];
  float wb_row = 0.0f;
  if constexpr (UPD) {   // (the parameter row, requested with everything else)
    if (wave == 0 && grp == 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        if (l16 + 16 * ch < W4) w_row[ch] = tbl_ld4<DT>(a.p.item_emb, (size_t)row * a.p.ld_item + 4 * (l16 + 16 * ch));
      if (l16 == 0) wb_row = a.p.item_b[(size_t)row * a.p.ld_itemb];
    }
  }
  double acc[NCH][4];
  zero_acc(acc);
  for (int k = off + gid; k < off + n; k += 16 * AP_OWN) {
    f32x4 v[AP_OWN][NCH];
#pragma unroll
    for (int u = 0; u < AP_OWN; ++u) {
      const int kk = k + 16 * u < off + n ? k + 16 * u : k;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        if (l16 + 16 * ch < W4) v[u][ch] = *(const f32x4*)(a.Gi + (size_t)kk * a.D + 4 * (l16 + 16 * ch));
    }
#pragma unroll
    for (int u = 0; u < AP_OWN; ++u)
      if (k + 16 * u < off + n) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          if (l16 + 16 * ch < W4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[ch][i] += exact_term(v[u][ch][i]);
          }
      }
  }
  double tb = 0.0;
  for (int k = off + tid; k < off + n; k += 256) tb += exact_term(a.Gb[k]);
  combine_groups(acc);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) tb += __shfl_xor(tb, o);
  if (grp == 0) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
      for (int i = 0; i < 4; ++i) shd[((wave * 16 + l16) * NCH + ch) * 4 + i] = acc[ch][i];
  }
  if (lane == 0) shp[wave] = tb;
  AP_SYNC();
  if constexpr (UPD) {
    const ApCtx& x = *xp;
    double part = 0.0;
    if (wave == 0 && grp == 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c4 = l16 + 16 * ch;
        if (c4 < W4) {
          const f32x4 w0 = w_row[ch];
          f32x4 wn;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            double s_ = 0.0;
            for (int w_ = 0; w_ < 4; ++w_) s_ += shd[((w_ * 16 + l16) * NCH + ch) * 4 + i];
            wn[i] = w0[i] - x.lazy_scale * (float)s_;      // (apply_elem<AP_UPDATE, lazy>)
          }
          tbl_st4<DT>(a.p.item_emb, (size_t)row * a.p.ld_item + 4 * c4, wn, x.salt ^ 0x85ebca6bu);
#pragma unroll
          for (int i = 0; i < 4; ++i) part += (double)wn[i] * (double)wn[i] - (double)w0[i] * (double)w0[i];
        }
      }
      if (l16 == 0) {
        const float gb = (float)((shp[0] + shp[1]) + (shp[2] + shp[3]));
        a.p.item_b[(size_t)row * a.p.ld_itemb] = wb_row - x.step * gb;    // not regularised, never scaled
        a.cnt_item[row] = 0;
      }
    }
    block_delta_store(part, shp, a, a.nbC + a.nbI + a.nbU + h, x.salt, x.accum);
    return;
  }
  if (wave == 0 && grp == 0) {
    const bool by_row = a.presum_rows != 0;
    float* R = by_row ? a.go.item_emb + (size_t)row * a.go.ld_item : a.Ri + (size_t)slot * a.di;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c4 = l16 + 16 * ch;
      if (c4 < W4) {
        f32x4 g;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double s = 0.0;
          for (int w_ = 0; w_ < 4; ++w_) s += shd[((w_ * 16 + l16) * NCH + ch) * 4 + i];
          g[i] = (float)s;
        }
        *(f32x4*)(R + 4 * c4) = g;
      }
    }
    if (l16 == 0) {
      const float gb = (float)((shp[0] + shp[1]) + (shp[2] + shp[3]));
      (by_row ? a.go.item_b[(size_t)row * a.go.ld_itemb] : a.Rb[slot]) = gb;
      a.cnt_item[row] = 0;
    }
    if (a.presum_rows == 2)
      for (int c = a.di + 1 + l16; c < a.go.ld_item; c += 16) R[c] = 0.0f;
  }
}

// WIDE: d_item / d_cate above 64 or d_item + Ls above 128 columns (more float4 chunks per lane)
template <int MODE, bool WIDE, int DT = TLSAN_TABLE_F32>
__global__ __launch_bounds__(256) void k_apply(ApplyArgs a) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  __shared__ double shd[4 * 16 * NC * 4];
  __shared__ double shp[4];
  __shared__ int sh_pos[AP_CAP];
  __shared__ int sh_lo[256], sh_n[256];
  __shared__ int sh_wtot[4];
  ApCtx x;
  x.tid = threadIdx.x; x.wave = x.tid >> 6; x.lane = x.tid & 63; x.grp = x.lane >> 4; x.l16 = x.lane & 15;
  x.gid = x.wave * 4 + x.grp;  // 16 groups
  x.blk = blockIdx.x;
  AP_STAMP(0);
  if (a.stamps != nullptr && x.tid == 0) a.stamps[(size_t)x.blk * 8 + 4] = __builtin_amdgcn_s_memrealtime();
  x.P = a.hdr->P;
  x.invP = 1.0f / x.P;
  x.step = MODE == AP_UPDATE ? a.lr * a.hdr->coef : 0.0f;
  x.lazy_scale = x.step / (x.P * (1.0f - x.step * a.reg));
  x.salt = a.hdr->nstep;
  x.coef = MODE == AP_UPDATE ? a.hdr->coef : 0.0f;
  if (MODE == AP_UPDATE && x.blk == 0 && x.tid == 0) a.hdr->spart_n[x.salt & 1] = a.nbC + a.nbI + a.nbU;
  x.oc.opt = a.opt; x.oc.lr = a.lr; x.oc.b1 = a.ob1; x.oc.b2 = a.ob2; x.oc.eps = a.oeps; x.oc.alpha = a.oalpha;
  const int blk = x.blk;
  if (blk < a.nbC) {
    if (a.cseg) apply_cseg_block<MODE, false, NC, AP_OWN, DT>(a, x, blk * AP_ROWS_PB, shp);   // (nbC = ceil(C / 16) then)
    else apply_cate_block<MODE, false, NC, DT>(a, x, shd, shp, sh_pos, sh_lo, sh_n, sh_wtot);
  } else if (blk < a.nbC + a.nbI) {
    apply_rows_block<MODE, false, true, NI, AP_OWN, DT>(a, x, (blk - a.nbC) * AP_ROWS_PB, shp);
  } else if (blk < a.nbC + a.nbI + a.nbU) {
    apply_rows_block<MODE, false, false, NU, AP_OWN / 2, DT>(a, x, (blk - a.nbC - a.nbI) * AP_ROWS_PB, shp);
  } else {
    // ================= 256 dense parameters =================
    const int nd = (blk - a.nbC - a.nbI - a.nbU) * 256 + x.tid;
    if constexpr (MODE == AP_UPDATE || MODE == AP_GRADS) {
      if (nd < a.lay.n_dense) {
        const float g = a.gd[nd];
        float w0 = 0.0f;
        if constexpr (MODE == AP_UPDATE) w0 = a.p.dense[nd];
        if constexpr (MODE == AP_GRADS) {
          a.go.dense[nd] = g;
        } else {
          float wn = w0 - x.step * g;
          if (a.opt != TLSAN_OPT_SGD) {
            float a1 = a.s1.dense[nd], a2 = a.s2.dense[nd];
            wn = w0;
            opt_elem(x.oc, wn, x.coef * g, a1, a2);
            a.s1.dense[nd] = a1; a.s2.dense[nd] = a2;
          }
          dense_store(a, nd, wn);
        }
      }
    }
  }
  AP_STAMP(6);
  // (slots 4/5: the device-wide 100 MHz clock at start/end; s_memtime is not synchronised across the chip)
  if (a.stamps != nullptr && x.tid == 0) a.stamps[(size_t)x.blk * 8 + 5] = __builtin_amdgcn_s_memrealtime();
}
#undef AP_STAMP

// tlsan_finalize_rows.h -- the dense finalize with row workgroups beside it, one unit per (d, heads) pair
// (tlsan_update_inst.h): k_finalize_presum (the row sums of the split lazy step) and k_finalize_update (the speculative
// one-pass lazy-L2 update).
#pragma once
#include "tlsan_finalize.h"
#include "tlsan_apply.h"

// ------------------------------------------------------------------------------------------
// The lazy-L2 train step splits the apply pass so that the row sums (which need neither the clip
// coefficient nor the dense gradients) overlap the dense finalize instead of waiting for it:
//   k_finalize_presum : workgroups [0, nbK+nbS] are k_dense_finalize's, the rest are k_apply's in
//                       PRESUM mode (exact per-row sums -> Rc / Ri / Rb / Ru, counters reset)
//   k_update_lazy     : elementwise w -= scale * sum for the used rows + the dense parameters
// Same arithmetic per element as apply_*_block<AP_UPDATE, lazy> (the sums are rounded to float there too).
// (the narrow form is held to 96 registers -- five workgroups per CU: left alone, the compiler takes 124 for the 64 loads the
//  dK entry blocks keep in flight and costs the launch a fifth of its residency; held, it needs 91 and spills nothing)
#ifndef PRESUM_WPE_WIDE
#define PRESUM_WPE_WIDE 4     // (128 registers, a few spilled in the wide row roles; three -- 138, nothing spilled -- measured slower: d = 256, Ls = 90 244.8 vs 238.5 us/step)
#endif
template <int D, int DH, bool WIDE, bool CSPLIT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WIDE ? PRESUM_WPE_WIDE : 5))) void k_finalize_presum(FinArgs f, int nbK, int nbS, ApplyArgs a) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  __shared__ double shd[4 * 16 * NC * 4 > 256 ? 4 * 16 * NC * 4 : 256];
  __shared__ double shp[4];
  __shared__ int sh_pos[AP_CAP];
  __shared__ int sh_lo[256], sh_n[256];
  __shared__ int sh_wtot[4];
  __shared__ int sh_last;
  const int nfin = nbK + nbS + 1;
  if ((int)blockIdx.x < nfin) {
    // (debug stamps: the finalize workgroups are listed after the apply workgroups)
    unsigned long long* stp = a.stamps ? a.stamps + (size_t)(gridDim.x - nfin + blockIdx.x) * 8 : nullptr;
    if (stp && threadIdx.x == 0) { stp[0] = __builtin_amdgcn_s_memtime(); stp[4] = __builtin_amdgcn_s_memrealtime(); }
    dense_finalize_block<D, DH>(f, nbK, nbS, blockIdx.x, shd, &sh_last);
    if (stp && threadIdx.x == 0) { stp[6] = __builtin_amdgcn_s_memtime(); stp[5] = __builtin_amdgcn_s_memrealtime(); }
    return;
  }
  ApCtx x = ap_ctx(a, nfin, 1.0f, 0.0f, 0u, 0.0f);
  if (x.blk < a.nbH) {   // hot item rows lead the grid (no debug stamps)
    presum_hot_block<NI>(a, x.blk, shd, shp);
    return;
  }
  x.blk -= a.nbH;
  unsigned long long* stp = a.stamps ? a.stamps + (size_t)x.blk * 8 : nullptr;
  if (stp && x.tid == 0) { stp[0] = __builtin_amdgcn_s_memtime(); stp[4] = __builtin_amdgcn_s_memrealtime(); }
  const int blk = x.blk;
  if (blk < a.nbC) {
    if (!CSPLIT && a.cseg) apply_cseg_block<AP_PRESUM, true, NC, AP_OWN, TLSAN_TABLE_F32>(a, x, blk * AP_ROWS_PB, shp);
    else apply_cate_block<AP_PRESUM, true, NC, TLSAN_TABLE_F32, CSPLIT>(a, x, shd, shp, sh_pos, sh_lo, sh_n, sh_wtot);
  }
  else if (blk < a.nbC + a.nbI) apply_rows_block<AP_PRESUM, true, true, NI, AP_OWN, TLSAN_TABLE_F32>(a, x, (blk - a.nbC) * AP_ROWS_PB, shp);
  else {
    apply_rows_block<AP_PRESUM, true, false, NU, AP_OWN / 2, TLSAN_TABLE_F32>(a, x, (blk - a.nbC - a.nbI) * AP_ROWS_PB, shp);
    if constexpr (!WIDE) {   // user rows wider than 128 floats with narrow item / category rows: the second half of the row
      if (a.WU > 128) apply_rows_block<AP_PRESUM, true, false, NU, AP_OWN / 2, TLSAN_TABLE_F32, NU>(a, x, (blk - a.nbC - a.nbI) * AP_ROWS_PB, shp);
    }
  }
  if (stp && x.tid == 0) { stp[6] = __builtin_amdgcn_s_memtime(); stp[5] = __builtin_amdgcn_s_memrealtime(); }
}

// ------------------------------------------------------------------------------------------
// The lazy-L2 step for tables that live in HBM (round 6): the SPECULATIVE one-pass update.
// The split form above sends every summed row through memory (written by the row-sum launch, read by k_update_lazy beside
// the parameter row's read-modify-write): at 10 M users / 5 M items that round trip is a third of the tail's traffic.  One
// pass over the used rows (segment sums and the row's update by the same lanes, apply_*_block<AP_UPDATE, lazy>) avoids it but
// needs the clip coefficient first, i.e. the finalize's whole chain in front of it (C5: 26 us).  clip_by_global_norm's
// coefficient is 1 unless the global norm exceeds the clip (model.py:201) -- so:
//   k_finalize_update : the finalize's workgroups lead the grid; the row workgroups update with coefficient 1 beside them.
//                       Neither P nor nstep change during the launch (FinArgs.spec): the summary leaves P_next / spec_salt.
//   k_spec_commit     : the dense parameters (which need the reduced gradients), the commit of P and nstep, and -- only if
//                       the coefficient turned out to be < 1 (or not finite) -- a correcting pass over the same rows:
//                       w += (scale_spec - scale_true) * sum, i.e. w_old - scale_true * sum up to one rounding.
// Unclipped steps are bit-equal to the one-pass form; results stay a fixed function of the batch.  Category segments only.
// (rows of tables with millions of rows are used once or twice per batch: two gradient rows in flight per 16-lane group
//  instead of AP_OWN = 8 clamped loads of the same row -- 60 registers fewer, five workgroups per CU instead of three;
//  longer segments are finished by the whole wavefront as everywhere, and the sums are exact: same bits)
// (the wide form -- rows of 128 floats and more, C5 -- is held to four waves per SIMD: 149 registers left alone, i.e. three;
//  at four 88 bytes per lane spill in the user-row role and C5 runs 281.5 -> 273.5 us/step.  The narrow form: five (fp32
//  tables) / four (bf16 tables) where the caches hold the tables -- the bench shape 56.9 -> 55.4 us/step against the split
//  form, at three it LOSES to it (59.3) --, three (LOWOCC) where they live in HBM: at d = 128 with 10 M / 5 M tables the step
//  is bound by the index stream, whose 1024-thread blocks find no slot beside five row workgroups per CU -- 80.5 us/step
//  with three, 92 with five: profiles/r06_lazy_one_pass.md)
#ifndef SPEC_WPE
#define SPEC_WPE 4
#endif
#ifndef SPEC_WPE_NARROW
#define SPEC_WPE_NARROW 5        // fp32 tables: 93 registers, nothing spilled
#define SPEC_WPE_NARROW_BF16 4   // bf16 tables (the stochastic rounding's hash): 113 registers; at five, 180 bytes per lane spill
#endif
// LOWOCC (narrow form, tables in HBM): three waves per SIMD -- see the note above
// CSPL (narrow form; few, large categories -- Movies-TV: 15 -- that several workgroups share, category_split): the category
// workgroups of this launch only SUM (exact doubles added into Rc64, as in k_finalize_presum<.., CSPLIT>) and the category
// rows are updated by k_spec_commit<.., CSPL>, which knows the coefficient; item and user rows as everywhere.  a.nbC is then
// the number of category-row blocks of the COMMIT launch (16 rows each: they own the records [0, nbC) of S_delta); this
// launch carries C * csplit category workgroups.  User rows of up to 256 floats (d = 128 with 90-entry windows) in two
// passes of the narrow form, as the row-sum launch takes them.
// The launch's ApplyArgs, dword by dword from the kernel-argument segment (KA: the kernel's parameters as a structure,
// which the segment lays out alike) to *dst: a correcting pass in a later launch reads them from there.  256 threads.
struct FinUpdateKernarg { FinArgs f; int nbK, nbS; ApplyArgs a; };
template <class KA>
__device__ __forceinline__ void keep_apply_args(void* dst) {
  typedef const uint32_t __attribute__((address_space(4))) * kword;
  const kword src = (kword)((const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(KA, a));
  for (int k = threadIdx.x; k < (int)(sizeof(ApplyArgs) / 4); k += 256) ((uint32_t*)dst)[k] = src[k];
}

template <int D, int DH, bool WIDE, int DT, bool LOWOCC = false, bool CSPL = false>
// (LOWOCC: three and no more -- the attribute's second number; 0 leaves the most open.  Left open, a build whose allocation
//  happens to fit 128 registers runs four)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WIDE ? SPEC_WPE : (LOWOCC ? 3 : (DT == TLSAN_TABLE_F32 ? SPEC_WPE_NARROW : SPEC_WPE_NARROW_BF16)), (!WIDE && LOWOCC) ? 3 : 0))) void k_finalize_update(FinArgs f, int nbK, int nbS, ApplyArgs a) {
  static_assert(!(WIDE && CSPL), "shared categories: narrow form only");
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  constexpr int OWN = WIDE ? SPEC_OWN : AP_OWN;
  __shared__ double shd[4 * 16 * NC * 4 > 256 ? 4 * 16 * NC * 4 : 256];
  __shared__ double shp[4];
  __shared__ int sh_pos[AP_CAP];
  __shared__ int sh_lo[256], sh_n[256];
  __shared__ int sh_wtot[4];
  __shared__ int sh_last;
  const int nfin = nbK + nbS + 1;
  if ((int)blockIdx.x < nfin) {
    // (debug stamps, scripts/stamps_apply.py: the finalize workgroups are listed after the row workgroups)
    unsigned long long* stp = a.stamps ? a.stamps + (size_t)(gridDim.x - nfin - a.nbH + blockIdx.x) * 8 : nullptr;
    if (stp && threadIdx.x == 0) { stp[0] = __builtin_amdgcn_s_memtime(); stp[4] = __builtin_amdgcn_s_memrealtime(); }
    dense_finalize_block<D, DH>(f, nbK, nbS, blockIdx.x, shd, &sh_last);
    if (stp && threadIdx.x == 0) { stp[6] = __builtin_amdgcn_s_memtime(); stp[5] = __builtin_amdgcn_s_memrealtime(); }
    return;
  }
  // P: stable (this launch's summary does not commit); step: coefficient 1; salt: what the step's salt and record tag
  // will be (hdr->spec_salt)
  // (two-launch form: this launch's summary DOES commit both -- k_fwd_bwd left their values at the step's start in the header)
  const bool two = a.fix_args != nullptr;
  ApCtx x = ap_ctx(a, nfin, *(two ? &a.hdr->P_snap : &a.hdr->P), a.lr, *(two ? &a.hdr->nstep_snap : &a.hdr->nstep) + 1, 1.0f);
  if (x.blk == 0 && x.tid == 0) a.hdr->spart_n[x.salt & 1] = a.nbC + a.nbI + a.nbU + a.nbH;
  if (two && x.blk == 0) keep_apply_args<FinUpdateKernarg>(a.fix_args);
  if (x.blk < a.nbH) {          // hot item rows lead the row workgroups
    presum_hot_block<NI, true, DT>(a, x.blk, shd, shp, &x);
    return;
  }
  x.blk -= a.nbH;
  unsigned long long* stp = a.stamps ? a.stamps + (size_t)x.blk * 8 : nullptr;
  if (stp && x.tid == 0) { stp[0] = __builtin_amdgcn_s_memtime(); stp[4] = __builtin_amdgcn_s_memrealtime(); }
  if constexpr (CSPL) {
    const int nbCg = a.C * a.csplit;       // category workgroups of this launch (category, share)
    if (x.blk < nbCg) {
      apply_cate_block<AP_PRESUM, true, NC, DT, true>(a, x, shd, shp, sh_pos, sh_lo, sh_n, sh_wtot);
    } else {
      // (the row blocks' records follow the commit launch's category blocks': [nbC | nbI | nbU].  Two-pass user blocks are the
      //  longer ones and lead the item blocks (a.ufirst) -- the launch ends when its last-placed blocks do)
      int rb = x.blk - nbCg;
      const int nbIl = a.nbI_l > 0 ? a.nbI_l : a.nbI;     // item-row workgroups launched (ApplyArgs.nbI_l)
      const bool uf = a.ufirst != 0;
      const bool is_user = uf ? rb < a.nbU : rb >= nbIl;
      if (is_user) rb -= uf ? 0 : nbIl; else rb -= uf ? a.nbU : 0;
      x.blk = a.nbC + (is_user ? a.nbI : 0) + rb;
      if (!is_user) {
        const int nuq = *a.n_uniq_item;
        for (int g = rb; g * AP_ROWS_PB < nuq && g < a.nbI; g += nbIl) {
          x.blk = a.nbC + g;
          apply_rows_block<AP_UPDATE, true, true, NI, OWN, DT>(a, x, g * AP_ROWS_PB, shp);
          __syncthreads();   // (the shared scratch is reused by the next block of rows)
        }
      } else {
        apply_rows_block<AP_UPDATE, true, false, NU, AP_OWN / 2, DT>(a, x, rb * AP_ROWS_PB, shp);
        if (a.WU > 128) {                    // the second half of a wide user row (its change of the sum of squares: added to the record)
          __syncthreads();
          x.accum = true;
          apply_rows_block<AP_UPDATE, true, false, NU, AP_OWN / 2, DT, NU>(a, x, rb * AP_ROWS_PB, shp);
        }
      }
    }
  } else {
    const int blk = x.blk;
    if (blk < a.nbC) {
      // (the wide form takes category segments only -- plan_tail, tlsan_api_plan.hip: the item-walk category workgroups in its
      //  kernel cost the row roles 44 more spilled bytes per lane)
      if (WIDE || a.cseg) apply_cseg_block<AP_UPDATE, true, NC, OWN, DT>(a, x, blk * AP_ROWS_PB, shp);
      else apply_cate_block<AP_UPDATE, true, NC, DT>(a, x, shd, shp, sh_pos, sh_lo, sh_n, sh_wtot);
    } else {
      // (records: [nbC | nbI | nbU] whatever the order of the workgroups.  The wide form's user rows -- 220 floats at C5,
      //  5.7-11 us a workgroup -- lead the item rows: placed last they WERE the launch's last 8 us: 60.5 -> 55)
      const int nbIl = a.nbI_l > 0 ? a.nbI_l : a.nbI;
      int rb = blk - a.nbC;
      const bool uf = a.ufirst != 0;
      const bool is_user = uf ? rb < a.nbU : rb >= nbIl;
      if (is_user) {
        rb -= uf ? 0 : nbIl;
        x.blk = a.nbC + a.nbI + rb;
        apply_rows_block<AP_UPDATE, true, false, NU, (WIDE ? SPEC_OWN : AP_OWN / 2), DT>(a, x, rb * AP_ROWS_PB, shp);
      } else {
        rb -= uf ? a.nbU : 0;
        const int nuq = *a.n_uniq_item;
        for (int g = rb; g * AP_ROWS_PB < nuq && g < a.nbI; g += nbIl) {
          x.blk = a.nbC + g;
          apply_rows_block<AP_UPDATE, true, true, NI, OWN, DT>(a, x, g * AP_ROWS_PB, shp);
          __syncthreads();   // (the shared scratch is reused by the next block of rows)
        }
      }
    }
  }
  if (stp && x.tid == 0) { stp[6] = __builtin_amdgcn_s_memtime(); stp[5] = __builtin_amdgcn_s_memrealtime(); }
}


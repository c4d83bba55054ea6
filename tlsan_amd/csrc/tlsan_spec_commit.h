// tlsan_spec_commit.h -- the launches behind k_finalize_update: k_spec_commit (the three-launch form's second launch) and
// k_spec_flush (the correction a clipped two-launch step owes when its successor has not run).  Instantiated in
// tlsan_update_d128.hip, beside k_finalize_update.
#pragma once
#include <type_traits>
#include "tlsan_finalize_rows.h"
#include "tlsan_fix.h"
#include "tlsan_lazy_rows.h"

// grid: nbD blocks of 256 dense parameters, (CSPL: a.nbC blocks of 16 category rows, updated here from the shared categories'
// exact sums with the step's true coefficient,) then at most SPEC_FIX_BLOCKS correcting workgroups (which return at once
// when the step was not clipped)
// (the narrow fp32 form at four waves per SIMD, as it has always run: two registers more and it would run at three)
template <bool WIDE, int DT, bool CSPL = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((!WIDE && DT == TLSAN_TABLE_F32) ? 4 : 2))) void k_spec_commit(ApplyArgs a) {
  constexpr int NC = WIDE ? 2 : 1, NI = WIDE ? 2 : 1, NU = WIDE ? 4 : 2;
  constexpr int OWN = WIDE ? SPEC_OWN : AP_OWN;
  __shared__ double shd[4 * 16 * NC * 4];
  __shared__ double shp[4];
  __shared__ int sh_pos[AP_CAP];
  __shared__ int sh_lo[256], sh_n[256];
  __shared__ int sh_wtot[4];
  const int tid = threadIdx.x;
  const float coef = a.hdr->coef;
  if ((int)blockIdx.x < a.nbD) {
    if (blockIdx.x == 0 && tid == 0) {   // (nothing in this launch reads P or nstep: P_prev / spec_salt hold what it needs)
      a.hdr->P = a.hdr->P_next;
      a.hdr->nstep += 1;
    }
    const float step = a.lr * coef;
    const int nd = blockIdx.x * 256 + tid;
    if (nd < a.lay.n_dense) dense_store(a, nd, a.p.dense[nd] - step * a.gd[nd]);
    return;
  }
  const float st_true = a.lr * coef;
  int fix0 = a.nbD;              // first correcting workgroup
  if constexpr (CSPL) {
    fix0 += a.nbC;
    if ((int)blockIdx.x < fix0) {   // 16 category rows: nothing speculative about them
      const float Pp = a.hdr->P_prev;
      const int cb = (int)blockIdx.x - a.nbD;
      const double part = update_cate_rows<NC, DT>(a, cb * 16 + (tid >> 4), tid & 15, st_true / (Pp * (1.0f - st_true * a.reg)), a.hdr->spec_salt);
      block_delta_store(part, shp, a, cb, a.hdr->spec_salt);
      return;
    }
  }
  if (coef == 1.0f) return;   // (block-uniform) the speculation held.  (A NaN coefficient takes the correcting pass and poisons the rows.)
  // (the launch carries at most SPEC_FIX_BLOCKS correcting workgroups, each walking row blocks with the grid's stride: an
  //  unclipped step -- nearly every step -- pays for a few hundred workgroups that return at once, not for one per 16 rows)
  [[maybe_unused]] const FixLds m = {shd, shp, sh_pos, sh_lo, sh_n, sh_wtot};
  ApCtx x = spec_fix_ctx(a);
  if constexpr (CSPL) {
    for (int v = (int)blockIdx.x - fix0; v < a.nbH + a.nbI + a.nbU; v += (int)gridDim.x - fix0) {
      if (v < a.nbH) {
        presum_hot_block<NI, true, DT>(a, v, shd, shp, &x);
      } else {
        const int rb = v - a.nbH;
        x.blk = a.nbC + rb;
        if (rb < a.nbI) {
          apply_rows_block<AP_UPDATE, true, true, NI, OWN, DT>(a, x, rb * AP_ROWS_PB, shp);
        } else {
          apply_rows_block<AP_UPDATE, true, false, NU, AP_OWN / 2, DT>(a, x, (rb - a.nbI) * AP_ROWS_PB, shp);
          if (a.WU > 128) {
            __syncthreads();
            apply_rows_block<AP_UPDATE, true, false, NU, AP_OWN / 2, DT, NU>(a, x, (rb - a.nbI) * AP_ROWS_PB, shp);
          }
        }
      }
      __syncthreads();
    }
  } else {
    spec_fix_blocks<WIDE, DT>(a, x, (int)blockIdx.x - a.nbD, (int)gridDim.x - a.nbD, false, m);
  }
}

// (keep_apply_args reads the launch's ApplyArgs at offsetof(FinUpdateKernarg, a): the structure has to list what the kernel takes)
static_assert(std::is_same<decltype(&k_finalize_update<128, 16, false, TLSAN_TABLE_F32>), void (*)(FinArgs, int, int, ApplyArgs)>::value &&
              std::is_same<decltype(FinUpdateKernarg::f), FinArgs>::value && std::is_same<decltype(FinUpdateKernarg::a), ApplyArgs>::value &&
              offsetof(FinUpdateKernarg, nbK) == sizeof(FinArgs) && offsetof(FinUpdateKernarg, nbS) == sizeof(FinArgs) + sizeof(int) &&
              offsetof(FinUpdateKernarg, a) == (sizeof(FinArgs) + 2 * sizeof(int) + alignof(ApplyArgs) - 1) / alignof(ApplyArgs) * alignof(ApplyArgs) &&
              sizeof(ApplyArgs) % 4 == 0,
              "FinUpdateKernarg mirrors k_finalize_update's parameters: edit both");

// The rare second half of the two-launch form outside the fused kernel (tlsan_state_flush): the correcting pass of a
// clipped step whose successor has not run -- before anything else reads the tables or the dense parameters.  The step's
// arguments come from the state (ApplyArgs.fix_args); the launch returns at once when nothing is pending, and its last
// workgroup, by ticket, says so.
template <bool WIDE, int DT>
__global__ __launch_bounds__(256) void k_spec_flush(const ApplyArgs* pa, StateHdr* hdr) {
  constexpr int NC = WIDE ? 2 : 1;
  static_assert(4 * 16 * NC * 4 <= FIX_SHD_DOUBLES, "FixLds: shd");
  __shared__ double shd[4 * 16 * NC * 4];
  __shared__ double shp[4];
  __shared__ int sh_pos[AP_CAP];
  __shared__ int sh_lo[256], sh_n[256];
  __shared__ int sh_wtot[4];
  if (hdr->fix_pending == 0) return;   // (grid-uniform: only the last workgroup to finish clears it)
  const FixLds m = {shd, shp, sh_pos, sh_lo, sh_n, sh_wtot};
  const ApplyArgs& a = *pa;
  ApCtx x = spec_fix_ctx(a);
  spec_fix_blocks<WIDE, DT>(a, x, (int)blockIdx.x, (int)gridDim.x, true, m);
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(&hdr->fix_ticket, 1) == (int)gridDim.x - 1) {
    hdr->fix_ticket = 0;
    hdr->fix_pending = 0;
  }
}

// tlsan_update_inst.h -- launchers of the dense finalize kernels (k_dense_finalize, k_finalize_presum,
// k_finalize_update), one template per (hidden_units, channels per head).  Every (d, heads) pair is instantiated in a
// unit of its own (tlsan_update_d*.hip), so that the six compile side by side; tlsan_api.hip reaches them through
// its table of pairs (g_pairs).
#pragma once
#include "tlsan_finalize_rows.h"

template <int D, int DH>
static void launch_finalize(const FinLaunch& L, hipStream_t hs) {
  const FinArgs& f = L.f;
  const ApplyArgs& A = L.A;
  const dim3 grid = L.grid, blk(256);
  const int nbK = L.nbK, nbS = L.nbS;
  if (L.kind == FinLaunch::UPDATE) {
    if (L.shared) {
      if (L.bf16) {
        if (L.low) hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_BF16, true, true>), grid, blk, 0, hs, f, nbK, nbS, A);
        else hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_BF16, false, true>), grid, blk, 0, hs, f, nbK, nbS, A);
      } else {
        if (L.low) hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_F32, true, true>), grid, blk, 0, hs, f, nbK, nbS, A);
        else hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_F32, false, true>), grid, blk, 0, hs, f, nbK, nbS, A);
      }
    } else if (L.bf16) {
      if (L.wide) hipLaunchKernelGGL((k_finalize_update<D, DH, true, TLSAN_TABLE_BF16>), grid, blk, 0, hs, f, nbK, nbS, A);
      else if (L.low) hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_BF16, true>), grid, blk, 0, hs, f, nbK, nbS, A);
      else hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_BF16>), grid, blk, 0, hs, f, nbK, nbS, A);
    } else {
      if (L.wide) hipLaunchKernelGGL((k_finalize_update<D, DH, true, TLSAN_TABLE_F32>), grid, blk, 0, hs, f, nbK, nbS, A);
      else if (L.low) hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_F32, true>), grid, blk, 0, hs, f, nbK, nbS, A);
      else hipLaunchKernelGGL((k_finalize_update<D, DH, false, TLSAN_TABLE_F32>), grid, blk, 0, hs, f, nbK, nbS, A);
    }
  } else if (L.kind == FinLaunch::PRESUM) {
    if (L.csplit) {
      if (L.wide) hipLaunchKernelGGL((k_finalize_presum<D, DH, true, true>), grid, blk, 0, hs, f, nbK, nbS, A);
      else hipLaunchKernelGGL((k_finalize_presum<D, DH, false, true>), grid, blk, 0, hs, f, nbK, nbS, A);
    } else if (L.wide) hipLaunchKernelGGL((k_finalize_presum<D, DH, true>), grid, blk, 0, hs, f, nbK, nbS, A);
    else hipLaunchKernelGGL((k_finalize_presum<D, DH, false>), grid, blk, 0, hs, f, nbK, nbS, A);
  } else {
    hipLaunchKernelGGL((k_dense_finalize<D, DH>), grid, blk, 0, hs, f, nbK, nbS);
  }
}

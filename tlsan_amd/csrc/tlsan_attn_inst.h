// tlsan_attn_inst.h -- per-D instantiation + launcher of k_fwd_bwd (one translation unit per D
// so the big kernels compile in parallel).
// A launch asks for the bytes of the kernel's own LDS layout (AttnLds, tlsan_attn_lds.h); the run-time choices of table
// storage, matrix products and dropout become template arguments in launch_variant / launch_variant_mm.
#pragma once
#include <atomic>
#include <hip/hip_ext.h>
#include "tlsan_attn.h"
#define TLSAN_MAX_DEVICES 16   // devices one process may drive (per-device launch attributes below)
struct LaunchEvents { hipEvent_t start, stop; };   // optional time stamps of the dispatch (tlsan_profile_*), or NULLs

template <int D, int DH, bool TRAIN, bool LSTREAM, int DT, bool DROP = false, int MM = TLSAN_MATRIX_F32, bool CSEG = false, int NWV = 0>
static hipError_t launch_variant_dt(const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  if constexpr (TRAIN && !CSEG) {   // tables with thousands of categories: the variant with category segments
    if (a.cseg) return launch_variant_dt<D, DH, TRAIN, LSTREAM, DT, DROP, MM, true, NWV>(a, grid, st, ev);
  }
  // (the byte count comes from the layout the kernel carves its pointers from: tlsan_attn_lds.h; a training launch's includes
  //  what the correcting pass at the kernel's head borrows, spec_fix_head -- every training form is far above that)
  const size_t smem = AttnLds<Geo<D, DH, NWV>, TRAIN, LSTREAM, DROP, CSEG>{0, a.b.Sn, a.fuse_dk != 0}.bytes();
  auto k = k_fwd_bwd<D, DH, TRAIN, LSTREAM, DT, DROP, MM, CSEG, NWV>;
  // (per kernel variant AND device: the attribute is raised once, not on every launch; relaxed atomics -- two threads
  //  racing on a first launch both raise it, which is harmless)
  static std::atomic<size_t> smem_set[TLSAN_MAX_DEVICES];
  if (smem > 48 * 1024) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<size_t>* slot = (dev >= 0 && dev < TLSAN_MAX_DEVICES) ? &smem_set[dev] : nullptr;
    if (slot == nullptr || smem > slot->load(std::memory_order_relaxed)) {
      (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (slot != nullptr) slot->store(smem, std::memory_order_relaxed);
    }
  }
  // (ev: optional pair of events attached to THIS dispatch -- its own begin / end time stamps, what a kernel trace
  //  reports -- instead of two events recorded around it, which are barrier packets of their own and read 3 us long)
  if (ev.start != nullptr) hipExtLaunchKernelGGL(k, dim3(grid), dim3(Geo<D, DH, NWV>::NW * 64), smem, st, ev.start, ev.stop, 0, a);
  else hipLaunchKernelGGL(k, dim3(grid), dim3(Geo<D, DH, NWV>::NW * 64), smem, st, a);
  return hipGetLastError();
}

// The run-time choices of a launch as template arguments, made here once: table storage and matrix products (fp32 / bf16,
// any pairing, either window form) ...
template <int D, int DH, bool TRAIN, bool LSTREAM, bool DROP, int NWV>
static hipError_t launch_variant_mm(const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  const bool tb = a.p.table_dtype == TLSAN_TABLE_BF16;
  if (a.p.matrix_dtype == TLSAN_MATRIX_BF16) {
    if (tb) return launch_variant_dt<D, DH, TRAIN, LSTREAM, TLSAN_TABLE_BF16, DROP, TLSAN_MATRIX_BF16, false, NWV>(a, grid, st, ev);
    return launch_variant_dt<D, DH, TRAIN, LSTREAM, TLSAN_TABLE_F32, DROP, TLSAN_MATRIX_BF16, false, NWV>(a, grid, st, ev);
  }
  if (tb) return launch_variant_dt<D, DH, TRAIN, LSTREAM, TLSAN_TABLE_BF16, DROP, TLSAN_MATRIX_F32, false, NWV>(a, grid, st, ev);
  return launch_variant_dt<D, DH, TRAIN, LSTREAM, TLSAN_TABLE_F32, DROP, TLSAN_MATRIX_F32, false, NWV>(a, grid, st, ev);
}
// ... and dropout (model.py:428-431): training only, and not as NWV-wavefront workgroups
template <int D, int DH, bool TRAIN, bool LSTREAM, int NWV = 0>
static hipError_t launch_variant(const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  if (a.drop_thr != 0) {
    if constexpr (TRAIN && NWV == 0) return launch_variant_mm<D, DH, TRAIN, LSTREAM, true, NWV>(a, grid, st, ev);
    else return hipErrorNotSupported;
  }
  return launch_variant_mm<D, DH, TRAIN, LSTREAM, false, NWV>(a, grid, st, ev);
}

template <int D, int DH>
static hipError_t launch_fwd_bwd_impl(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  if (train) return lstream ? launch_variant<D, DH, true, true>(a, grid, st, ev) : launch_variant<D, DH, true, false>(a, grid, st, ev);
  return lstream ? launch_variant<D, DH, false, true>(a, grid, st, ev) : launch_variant<D, DH, false, false>(a, grid, st, ev);
}

// one window form only (a translation unit of its own for the streamed form of d = 256, which is compiled with other flags)
template <int D, int DH, bool LSTREAM>
static hipError_t launch_fwd_bwd_form(bool train, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  if (train) return launch_variant<D, DH, true, LSTREAM>(a, grid, st, ev);
  return launch_variant<D, DH, false, LSTREAM>(a, grid, st, ev);
}

// training step with the window in registers, no dropout, as NWV-wavefront workgroups (d = 128: 4 wavefronts, 8 samples)
template <int D, int DH, int NWV>
static hipError_t launch_train_nw(const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  return launch_variant<D, DH, true, false, NWV>(a, grid, st, ev);
}

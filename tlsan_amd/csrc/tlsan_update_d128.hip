// dense finalize kernels (tlsan_update_inst.h) for hidden_units = 128 with 8 heads (16 channels per head)
#include "tlsan_update_inst.h"
#include "tlsan_spec_commit.h"
void tlsan_launch_finalize_d128(const FinLaunch& L, hipStream_t hs) { launch_finalize<128, 16>(L, hs); }

// ... and k_spec_commit of every pair: compiled beside k_finalize_update, whose row helpers it shares -- alone in a unit the
// inliner takes them in another order and the narrow fp32 form needs 129 registers instead of 127: three waves per SIMD, not four
void tlsan_launch_spec_commit(bool wide, bool bf16, bool shared, dim3 grid, const ApplyArgs& A, hipStream_t hs) {
  const dim3 blk(256);
  if (shared) {
    if (bf16) hipLaunchKernelGGL((k_spec_commit<false, TLSAN_TABLE_BF16, true>), grid, blk, 0, hs, A);
    else hipLaunchKernelGGL((k_spec_commit<false, TLSAN_TABLE_F32, true>), grid, blk, 0, hs, A);
  } else if (bf16 && wide) hipLaunchKernelGGL((k_spec_commit<true, TLSAN_TABLE_BF16>), grid, blk, 0, hs, A);
  else if (bf16) hipLaunchKernelGGL((k_spec_commit<false, TLSAN_TABLE_BF16>), grid, blk, 0, hs, A);
  else if (wide) hipLaunchKernelGGL((k_spec_commit<true, TLSAN_TABLE_F32>), grid, blk, 0, hs, A);
  else hipLaunchKernelGGL((k_spec_commit<false, TLSAN_TABLE_F32>), grid, blk, 0, hs, A);
}

void tlsan_launch_spec_flush(bool wide, bool bf16, const void* args, void* hdr, hipStream_t hs) {
  const dim3 grid(256), blk(256);   // (each workgroup walks the row blocks with the grid's stride: spec_fix_blocks)
  const ApplyArgs* pa = (const ApplyArgs*)args;
  StateHdr* h = (StateHdr*)hdr;
  if (bf16 && wide) hipLaunchKernelGGL((k_spec_flush<true, TLSAN_TABLE_BF16>), grid, blk, 0, hs, pa, h);
  else if (bf16) hipLaunchKernelGGL((k_spec_flush<false, TLSAN_TABLE_BF16>), grid, blk, 0, hs, pa, h);
  else if (wide) hipLaunchKernelGGL((k_spec_flush<true, TLSAN_TABLE_F32>), grid, blk, 0, hs, pa, h);
  else hipLaunchKernelGGL((k_spec_flush<false, TLSAN_TABLE_F32>), grid, blk, 0, hs, pa, h);
}

// k_fwd_bwd instantiations for hidden_units = 64 with 4 heads (16 channels per head)
#include "tlsan_attn_inst.h"
hipError_t tlsan_launch_fwd_bwd_d64h4(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  return launch_fwd_bwd_impl<64, 16>(train, lstream, a, grid, st, ev);
}

// k_fwd_bwd instantiations for hidden_units = 128 with 16 heads (8 channels per head)
#include "tlsan_attn_inst.h"
hipError_t tlsan_launch_fwd_bwd_d128h16(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev) {
  return launch_fwd_bwd_impl<128, 8>(train, lstream, a, grid, st, ev);
}

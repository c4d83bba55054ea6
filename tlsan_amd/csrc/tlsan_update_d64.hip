// dense finalize kernels (tlsan_update_inst.h) for hidden_units = 64 with 8 heads (8 channels per head)
#include "tlsan_update_inst.h"
void tlsan_launch_finalize_d64(const FinLaunch& L, hipStream_t hs) { launch_finalize<64, 8>(L, hs); }

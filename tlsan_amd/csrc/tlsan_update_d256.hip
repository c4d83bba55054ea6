// dense finalize kernels (tlsan_update_inst.h) for hidden_units = 256 with 8 heads (32 channels per head)
#include "tlsan_update_inst.h"
void tlsan_launch_finalize_d256(const FinLaunch& L, hipStream_t hs) { launch_finalize<256, 32>(L, hs); }

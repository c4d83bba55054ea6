// dense finalize kernels (tlsan_update_inst.h) for hidden_units = 128 with 4 heads (32 channels per head)
#include "tlsan_update_inst.h"
void tlsan_launch_finalize_d128h4(const FinLaunch& L, hipStream_t hs) { launch_finalize<128, 32>(L, hs); }

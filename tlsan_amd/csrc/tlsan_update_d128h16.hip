// dense finalize kernels (tlsan_update_inst.h) for hidden_units = 128 with 16 heads (8 channels per head)
#include "tlsan_update_inst.h"
void tlsan_launch_finalize_d128h16(const FinLaunch& L, hipStream_t hs) { launch_finalize<128, 8>(L, hs); }

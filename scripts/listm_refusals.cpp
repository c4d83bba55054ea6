// The refusals of tlsan_list_metrics as a stand-alone host program, for a sanitizer run of the entry point's host side
// (tlsan_listm.hip: argument checks and launcher) without Python and without a GPU: every call below must be refused
// before any launch, on fake pointers that are never dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_listm.hip scripts/listm_refusals.cpp -o listm_refusals && ./listm_refusals
// fail() and tlsan_last_error() live in tlsan_api.hip in the library; this program brings its own copies.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "tlsan.h"

static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
extern "C" const char* tlsan_last_error(void) { return g_err; }

struct Call {
  const void* p[10];   // ids vec inv cate n_valid pair_cos n_cate max_cate hit_pos weight_sum
  const void* exposure;
  int32_t B, K, d, n_items;
};

static int run(const Call& c) {
  return tlsan_list_metrics((const int32_t*)c.p[0], (const float*)c.p[1], (const float*)c.p[2], (const int32_t*)c.p[3], nullptr,
                            nullptr, c.B, c.K, c.d, (int32_t*)c.p[4], (double*)c.p[5], (int32_t*)c.p[6], (int32_t*)c.p[7],
                            (int32_t*)c.p[8], (double*)c.p[9], (uint32_t*)c.exposure, c.n_items, nullptr);
}

static int bad = 0;
static void expect(const char* what, const Call& c, int code, const char* in_message) {
  const int rc = run(c);
  const bool ok = rc == code && strstr(tlsan_last_error(), in_message) != nullptr;
  printf("%-34s rc %d  \"%s\"  %s\n", what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
  bad += !ok;
}

int main() {
  const void* fake = (const void*)0x1000;
  Call good;
  for (auto& q : good.p) q = fake;
  good.exposure = nullptr;
  good.B = 3; good.K = 10; good.d = 64; good.n_items = 0;
  Call c = good; c.B = 0;               expect("B = 0", c, TLSAN_E_BADARG, "tlsan_list_metrics: B");
  c = good; c.B = 1 << 24; c.K = 256;   expect("B * K = 2^32", c, TLSAN_E_BADARG, "tlsan_list_metrics: B");
  c = good; c.K = 0;                    expect("K = 0", c, TLSAN_E_BADARG, "tlsan_list_metrics: K");
  c = good; c.K = 257;                  expect("K = 257", c, TLSAN_E_BADARG, "tlsan_list_metrics: K");
  c = good; c.d = 96;                   expect("d = 96", c, TLSAN_E_UNSUPPORTED, "tlsan_list_metrics: d");
  c = good; c.exposure = fake;          expect("exposure with n_items = 0", c, TLSAN_E_BADARG, "tlsan_list_metrics: exposure");
  c.n_items = -3;                       expect("exposure with n_items = -3", c, TLSAN_E_BADARG, "tlsan_list_metrics: exposure");
  for (int hole = 0; hole < 10; ++hole) {
    c = good; c.p[hole] = nullptr;
    char what[40];
    snprintf(what, sizeof(what), "pointer %d NULL", hole);
    expect(what, c, TLSAN_E_BADARG, "tlsan_list_metrics: NULL");
  }
  printf(bad ? "%d refusals WRONG\n" : "all refusals as specified\n", bad);
  return bad != 0;
}

// The refusals of tlsan_dense_topk_workspace_bytes and tlsan_dense_topk as a stand-alone host program, for a sanitizer run
// of the entry points' host side (tlsan_dense.hip: argument checks and workspace carve-up) without Python and without a
// GPU: every call below must be refused before any launch, on fake pointers that are never dereferenced.  From the
// repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_dense.hip -x hip scripts/audience_refusals.cpp -o audience_refusals && ./audience_refusals
// What tlsan_dense.hip takes from the other units of the library this program brings itself: fail() and
// tlsan_last_error(), and a stand-in for the merge's launcher, which no refused call reaches (it aborts if one does).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tlsan_host.h"

static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
extern "C" const char* tlsan_last_error(void) { return g_err; }

hipError_t tlsan_launch_topk_merge(const int32_t*, const float*, int, int, int, int32_t*, float*, hipStream_t) {
  printf("a refused call reached a launcher\n");
  abort();
}

static void* const FAKE = (void*)0x1000;
static int bad = 0;

static void expect(const char* what, int rc, int code) {
  static const char* fn = "tlsan_dense_topk:";
  const bool ok = rc == code && strstr(tlsan_last_error(), fn) == tlsan_last_error();
  printf("%-34s rc %d  \"%s\"  %s\n", what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
  bad += !ok;
}

static size_t size_of(const char* what, int32_t Q, int32_t N, int32_t K, bool zero) {
  g_err[0] = 0;
  const size_t n = tlsan_dense_topk_workspace_bytes(Q, N, K);
  const bool ok = zero ? (n == 0 && strstr(tlsan_last_error(), "tlsan_dense_topk_workspace_bytes") == tlsan_last_error()) : n > 0;
  printf("workspace_bytes %-26s %zu bytes  %s\n", what, n, ok ? "ok" : "WRONG");
  bad += !ok;
  return n;
}

struct Call {
  const void* q; int32_t Q, d; const void* x; int32_t N; const void *scale, *bias, *off, *xid; int32_t id_add, K;
  void *ids, *scores, *ws; size_t ws_bytes;
};
static int run(const Call& c) {
  return tlsan_dense_topk((const float*)c.q, c.Q, c.d, (const float*)c.x, c.N, (const float*)c.scale, (const float*)c.bias,
                          (const int32_t*)c.off, (const int32_t*)c.xid, c.id_add, c.K, (int32_t*)c.ids, (float*)c.scores, c.ws,
                          c.ws_bytes, nullptr);
}

int main() {
  size_of("one query, one row", 1, 1, 1, false);
  size_of("16 queries, 10 M rows, K 256", 16, 10000000, 256, false);
  size_of("the largest call", 1 << 24, 1 << 30, 256, false);
  // never less for a larger Q, N or K (the slice count itself falls as the query tiles fill the chip)
  const int32_t Qs[] = {1, 16, 17, 32, 33, 48, 49, 256, 4096, 4097, 1 << 20}, Ns[] = {1, 256, 257, 600, 200000, 1 << 30};
  for (int32_t K : {1, 16, 17, 64, 65, 256})
    for (int32_t N : Ns) {
      size_t prev = 0;
      for (int32_t Q : Qs) {
        const size_t n = tlsan_dense_topk_workspace_bytes(Q, N, K);
        if (n == 0 || n < prev) { printf("not monotone in Q at (%d, %d, %d)  WRONG\n", Q, N, K); ++bad; }
        prev = n;
      }
    }
  size_of("Q = 0", 0, 10, 1, true);
  size_of("Q = -1", -1, 10, 1, true);
  size_of("Q = 2^24 + 1", (1 << 24) + 1, 10, 1, true);
  size_of("N = 0", 4, 0, 1, true);
  size_of("N = -7", 4, -7, 1, true);
  size_of("N = 2^30 + 1", 4, (1 << 30) + 1, 1, true);
  size_of("K = 0", 4, 10, 0, true);
  size_of("K = 257", 4, 10, 257, true);

  const size_t need = tlsan_dense_topk_workspace_bytes(40, 600, 10);
  const Call g = {FAKE, 40, 128, FAKE, 600, nullptr, nullptr, nullptr, nullptr, 0, 10, FAKE, FAKE, FAKE, need};
  Call c = g; c.q = nullptr;                        expect("q NULL", run(c), TLSAN_E_BADARG);
  c = g; c.x = nullptr;                             expect("x NULL", run(c), TLSAN_E_BADARG);
  c = g; c.ids = nullptr;                           expect("ids NULL", run(c), TLSAN_E_BADARG);
  c = g; c.scores = nullptr;                        expect("scores NULL", run(c), TLSAN_E_BADARG);
  c = g; c.ws = nullptr;                            expect("ws NULL", run(c), TLSAN_E_WORKSPACE);
  c = g; c.off = FAKE;                              expect("excl_off without excl_ids", run(c), TLSAN_E_BADARG);
  c = g; c.xid = FAKE;                              expect("excl_ids without excl_off", run(c), TLSAN_E_BADARG);
  c = g; c.Q = 0;                                   expect("Q = 0", run(c), TLSAN_E_BADARG);
  c = g; c.Q = -5;                                  expect("Q = -5", run(c), TLSAN_E_BADARG);
  c = g; c.N = 0;                                   expect("N = 0", run(c), TLSAN_E_BADARG);
  c = g; c.N = -1;                                  expect("N = -1", run(c), TLSAN_E_BADARG);
  c = g; c.N = INT32_MAX;                           expect("N = 2^31 - 1", run(c), TLSAN_E_BADARG);
  c = g; c.id_add = INT32_MAX - 598;                expect("id_add + N = 2^31 + 1", run(c), TLSAN_E_BADARG);
  c = g; c.N = 1 << 30; c.id_add = (1 << 30) + 1; c.ws_bytes = (size_t)1 << 62;
  expect("N = 2^30, id_add + N past int32", run(c), TLSAN_E_BADARG);
  c = g; c.id_add = -1;                             expect("id_add = -1", run(c), TLSAN_E_BADARG);
  c = g; c.d = 96;                                  expect("d = 96", run(c), TLSAN_E_UNSUPPORTED);
  c = g; c.d = 0;                                   expect("d = 0", run(c), TLSAN_E_UNSUPPORTED);
  c = g; c.d = 512;                                 expect("d = 512", run(c), TLSAN_E_UNSUPPORTED);
  c = g; c.K = 0;                                   expect("K = 0", run(c), TLSAN_E_BADARG);
  c = g; c.K = 257;                                 expect("K = 257", run(c), TLSAN_E_BADARG);
  c = g; c.ws_bytes = need - 1;                     expect("ws one byte short", run(c), TLSAN_E_WORKSPACE);
  c = g; c.ws_bytes = 0;                            expect("no workspace", run(c), TLSAN_E_WORKSPACE);
  c = g; c.Q = 1 << 24; c.N = 1 << 30; c.K = 256; c.ws_bytes = 1 << 20;
  expect("the largest call, 1 MiB", run(c), TLSAN_E_WORKSPACE);

  printf(bad ? "%d refusals WRONG\n" : "all refusals as specified\n", bad);
  return bad != 0;
}

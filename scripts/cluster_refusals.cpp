// The refusals of tlsan_cluster_workspace_bytes, tlsan_cluster_assign, tlsan_cluster_means and tlsan_cluster_probe as a
// stand-alone host program, for a sanitizer run of the entry points' host side (tlsan_cluster.hip: argument checks) without
// Python and without a GPU: every call below must be refused before any launch, on fake pointers that are never
// dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_cluster.hip -x hip scripts/cluster_refusals.cpp -o cluster_refusals && ./cluster_refusals
// What tlsan_cluster.hip takes from the other units of the library this program brings itself: fail() and tlsan_last_error().
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

static void* const FAKE = (void*)0x1000;
static int bad = 0;

static void expect(const char* fn, const char* what, int rc, int code) {
  const bool ok = rc == code && strstr(tlsan_last_error(), fn) == tlsan_last_error();
  printf("%-22s %-26s rc %d  \"%s\"  %s\n", fn, what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
  bad += !ok;
}

static void expect_size(const char* what, int32_t B, int32_t C, int32_t P, bool zero) {
  const size_t n = tlsan_cluster_workspace_bytes(B, C, P);
  const bool ok = zero ? (n == 0 && strstr(tlsan_last_error(), "tlsan_cluster_workspace_bytes") == tlsan_last_error()) : n > 0;
  printf("%-22s %-26s %zu bytes  %s\n", "workspace_bytes", what, n, ok ? "ok" : "WRONG");
  bad += !ok;
}

struct Assign {
  const void* x; int32_t N, d; const void* cent; int32_t C; void *assign, *dist, *ws; size_t ws_bytes;
};
static int run(const Assign& a) {
  return tlsan_cluster_assign((const float*)a.x, a.N, a.d, (const float*)a.cent, a.C, (int32_t*)a.assign, (float*)a.dist, a.ws,
                              a.ws_bytes, nullptr);
}

struct Means {
  const void* x; int32_t N; const void *order, *seg; int32_t C, d; void* cent;
};
static int run(const Means& m) {
  return tlsan_cluster_means((const float*)m.x, m.N, (const int32_t*)m.order, (const int32_t*)m.seg, m.C, m.d, (float*)m.cent,
                             nullptr);
}

struct Probe {
  const void* q; int32_t B, d; const void *cent, *scale, *bias, *off; int32_t C, P; void *rows, *ws; size_t ws_bytes;
};
static int run(const Probe& p) {
  return tlsan_cluster_probe((const float*)p.q, p.B, p.d, (const float*)p.cent, (const float*)p.scale, (const float*)p.bias,
                             (const int32_t*)p.off, p.C, p.P, (int32_t*)p.rows, p.ws, p.ws_bytes, nullptr);
}

int main() {
  expect_size("assign alone", 0, 16384, 0, false);
  expect_size("assign and probe", 4096, 1024, 64, false);
  expect_size("C = 0", 4, 0, 2, true);
  expect_size("C = 16385", 4, 16385, 2, true);
  expect_size("P = 65", 4, 10, 65, true);
  expect_size("P = -1", 4, 10, -1, true);
  expect_size("B = -1", -1, 10, 2, true);
  expect_size("B * P past int32", 1 << 30, 10, 64, true);

  const char* fa = "tlsan_cluster_assign";
  const Assign ga = {FAKE, 100, 128, FAKE, 10, FAKE, FAKE, FAKE, (size_t)1 << 30};
  Assign a = ga; a.x = nullptr;                   expect(fa, "x NULL", run(a), TLSAN_E_BADARG);
  a = ga; a.cent = nullptr;                       expect(fa, "cent NULL", run(a), TLSAN_E_BADARG);
  a = ga; a.assign = nullptr;                     expect(fa, "assign NULL", run(a), TLSAN_E_BADARG);
  a = ga; a.d = 96;                               expect(fa, "d = 96", run(a), TLSAN_E_UNSUPPORTED);
  a = ga; a.d = 0;                                expect(fa, "d = 0", run(a), TLSAN_E_UNSUPPORTED);
  a = ga; a.N = 0;                                expect(fa, "N = 0", run(a), TLSAN_E_BADARG);
  a = ga; a.N = -3;                               expect(fa, "N = -3", run(a), TLSAN_E_BADARG);
  a = ga; a.C = 0;                                expect(fa, "C = 0", run(a), TLSAN_E_BADARG);
  a = ga; a.C = 16385;                            expect(fa, "C = 16385", run(a), TLSAN_E_BADARG);
  a = ga; a.ws = nullptr;                         expect(fa, "ws NULL", run(a), TLSAN_E_WORKSPACE);
  a = ga; a.ws_bytes = tlsan_cluster_workspace_bytes(0, 10, 0) - 1;
  expect(fa, "ws one byte short", run(a), TLSAN_E_WORKSPACE);
  a = ga; a.ws_bytes = 0;                         expect(fa, "no workspace", run(a), TLSAN_E_WORKSPACE);

  const char* fm = "tlsan_cluster_means";
  const Means gm = {FAKE, 100, FAKE, FAKE, 10, 128, FAKE};
  Means m = gm; m.x = nullptr;                    expect(fm, "x NULL", run(m), TLSAN_E_BADARG);
  m = gm; m.order = nullptr;                      expect(fm, "order NULL", run(m), TLSAN_E_BADARG);
  m = gm; m.seg = nullptr;                        expect(fm, "seg_off NULL", run(m), TLSAN_E_BADARG);
  m = gm; m.cent = nullptr;                       expect(fm, "cent NULL", run(m), TLSAN_E_BADARG);
  m = gm; m.d = 32;                               expect(fm, "d = 32", run(m), TLSAN_E_UNSUPPORTED);
  m = gm; m.N = 0;                                expect(fm, "N = 0", run(m), TLSAN_E_BADARG);
  m = gm; m.C = 0;                                expect(fm, "C = 0", run(m), TLSAN_E_BADARG);
  m = gm; m.C = 16385;                            expect(fm, "C = 16385", run(m), TLSAN_E_BADARG);

  const char* fp = "tlsan_cluster_probe";
  const Probe gp = {FAKE, 48, 128, FAKE, nullptr, nullptr, nullptr, 10, 8, FAKE, FAKE, (size_t)1 << 30};
  Probe p = gp; p.q = nullptr;                    expect(fp, "q NULL", run(p), TLSAN_E_BADARG);
  p = gp; p.cent = nullptr;                       expect(fp, "cent NULL", run(p), TLSAN_E_BADARG);
  p = gp; p.rows = nullptr;                       expect(fp, "row_lists NULL", run(p), TLSAN_E_BADARG);
  p = gp; p.d = 512;                              expect(fp, "d = 512", run(p), TLSAN_E_UNSUPPORTED);
  p = gp; p.B = 0;                                expect(fp, "B = 0", run(p), TLSAN_E_BADARG);
  p = gp; p.B = (1 << 24) + 1;                    expect(fp, "B = 2^24 + 1", run(p), TLSAN_E_BADARG);
  p = gp; p.C = 0;                                expect(fp, "C = 0", run(p), TLSAN_E_BADARG);
  p = gp; p.C = 16385;                            expect(fp, "C = 16385", run(p), TLSAN_E_BADARG);
  p = gp; p.P = 0;                                expect(fp, "P = 0", run(p), TLSAN_E_BADARG);
  p = gp; p.P = 65;                               expect(fp, "P = 65", run(p), TLSAN_E_BADARG);
  p = gp; p.ws = nullptr;                         expect(fp, "ws NULL", run(p), TLSAN_E_WORKSPACE);
  p = gp; p.ws_bytes = 48 * 8 * 4 - 1;            expect(fp, "ws one byte short", run(p), TLSAN_E_WORKSPACE);
  p = gp; p.B = 1 << 24; p.P = 64; p.ws_bytes = 1 << 20;
  expect(fp, "the largest call, 1 MiB", run(p), TLSAN_E_WORKSPACE);

  printf(bad ? "%d refusals WRONG\n" : "all refusals as specified\n", bad);
  return bad != 0;
}

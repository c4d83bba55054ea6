// The workspace sizes and the refusals of tlsan_shortlist_build, tlsan_shortlist_workspace_bytes, tlsan_shortlist_topk and
// tlsan_shortlist_select as a stand-alone host program, for a sanitizer run of the entry points' host side
// (tlsan_shortlist.hip: argument checks, the slicing and the workspace carve-up) without Python and without a GPU: every call
// below must be refused before any launch, on fake pointers that are never dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_shortlist.hip -x hip scripts/shortlist_refusals.cpp -o shortlist_refusals && ./shortlist_refusals
// What tlsan_shortlist.hip takes from the other units of the library this program brings itself: fail() and tlsan_last_error().
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
  printf("%-24s %-30s rc %d  \"%s\"  %s\n", fn, what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
  bad += !ok;
}

static void expect_size(const char* what, int32_t I, int32_t B, int32_t d, int32_t N, bool zero, size_t at_least) {
  const size_t n = tlsan_shortlist_workspace_bytes(I, B, d, N);
  const bool ok = zero ? (n == 0 && strstr(tlsan_last_error(), "tlsan_shortlist_workspace_bytes") == tlsan_last_error())
                       : (n > 0 && n >= at_least);
  printf("%-24s %-30s %zu bytes  %s\n", "workspace_bytes", what, n, ok ? "ok" : "WRONG");
  bad += !ok;
}

struct Build {
  const tlsan_dims* dims; const tlsan_params* p; void *vec, *wmax;
};
static int run(const Build& b) { return tlsan_shortlist_build(b.dims, b.p, (uint16_t*)b.vec, (float*)b.wmax, nullptr); }

struct Topk {
  const void* vec; int32_t I, d; const void* u_t; int32_t B; const void *scale, *item_b; int32_t ld, N; const void *xo, *xi;
  int32_t mul, add; void *ids, *approx, *ws; size_t ws_bytes;
};
static int run(const Topk& t) {
  return tlsan_shortlist_topk((const uint16_t*)t.vec, t.I, t.d, (const float*)t.u_t, t.B, (const float*)t.scale,
                              (const float*)t.item_b, t.ld, t.N, (const int32_t*)t.xo, (const int32_t*)t.xi, t.mul, t.add,
                              (int32_t*)t.ids, (float*)t.approx, t.ws, t.ws_bytes, nullptr);
}

struct Select {
  const void *sid, *exact, *approx, *u_t, *scale, *wmax; int32_t B, d, N, K; void *ids, *scores, *cert;
};
static int run(const Select& s) {
  return tlsan_shortlist_select((const int32_t*)s.sid, (const float*)s.exact, (const float*)s.approx, (const float*)s.u_t,
                                (const float*)s.scale, (const float*)s.wmax, s.B, s.d, s.N, s.K, (int32_t*)s.ids,
                                (float*)s.scores, (int32_t*)s.cert, nullptr);
}

int main() {
  // one slice writes the result itself: nothing is carved, yet the size is not 0 (0 is a refusal's)
  expect_size("one slice", 15, 1, 64, 16, false, 1);
  // 4096 rows over 5 M items: 128 row groups of 32 rows (two tiles of 16), so 2048 / 128 = 16 slices of [B, N] ids and scores
  expect_size("5 M items, 4096 rows", 5000000, 4096, 128, 64, false, (size_t)2 * 4 * 4096 * 16 * 64);
  // ... and no more than that and the 256 bytes every size carries: the slices follow the row groups the kernel is built with
  {
    const size_t n = tlsan_shortlist_workspace_bytes(5000000, 4096, 128, 64), want = (size_t)2 * 4 * 4096 * 16 * 64 + 256;
    printf("%-24s %-30s %zu bytes (want %zu)  %s\n", "workspace_bytes", "5 M items, exactly", n, want, n == want ? "ok" : "WRONG");
    bad += n != want;
  }
  expect_size("the longest shortlist", 5000000, 4096, 256, 256, false, (size_t)2 * 4 * 4096 * 256);
  expect_size("2^22 rows of 256", 1 << 30, 1 << 22, 256, 256, false, 1);
  expect_size("B * N = 2^31", 1 << 30, 1 << 23, 256, 256, true, 0);
  expect_size("d = 96", 100, 4, 96, 64, true, 0);
  expect_size("d = 0", 100, 4, 0, 64, true, 0);
  expect_size("N = 15", 100, 4, 128, 15, true, 0);
  expect_size("N = 257", 100, 4, 128, 257, true, 0);
  expect_size("I = 0", 0, 4, 128, 64, true, 0);
  expect_size("I = 2^30 + 1", (1 << 30) + 1, 4, 128, 64, true, 0);
  expect_size("B = 0", 100, 0, 128, 64, true, 0);
  expect_size("B = 2^24 + 1", 100, (1 << 24) + 1, 128, 64, true, 0);

  const char* fb = "tlsan_shortlist_build";
  tlsan_dims gd;
  memset(&gd, 0, sizeof(gd));
  gd.user_count = 10; gd.item_count = 100; gd.cate_count = 5; gd.d = 128; gd.d_item = 64; gd.d_cate = 64; gd.num_heads = 8; gd.Ls = 10;
  tlsan_params gp;
  memset(&gp, 0, sizeof(gp));
  gp.item_emb = (float*)FAKE; gp.cate_emb = (float*)FAKE; gp.item_cate = (const int32_t*)FAKE; gp.item_b = (float*)FAKE;
  const Build gb = {&gd, &gp, FAKE, FAKE};
  Build b = gb; b.dims = nullptr;                  expect(fb, "dims NULL", run(b), TLSAN_E_BADARG);
  b = gb; b.p = nullptr;                           expect(fb, "p NULL", run(b), TLSAN_E_BADARG);
  b = gb; b.vec = nullptr;                         expect(fb, "vec NULL", run(b), TLSAN_E_BADARG);
  b = gb; b.wmax = nullptr;                        expect(fb, "wmax NULL", run(b), TLSAN_E_BADARG);
  tlsan_dims d2 = gd; d2.d = 96; d2.d_item = 48; d2.d_cate = 48; b = gb; b.dims = &d2;
  expect(fb, "d = 96", run(b), TLSAN_E_UNSUPPORTED);
  d2 = gd; d2.d_item = 62; d2.d_cate = 66;         expect(fb, "d_item = 62", run(b), TLSAN_E_BADARG);
  d2 = gd; d2.d_cate = 32;                         expect(fb, "d_item + d_cate != d", run(b), TLSAN_E_BADARG);
  d2 = gd; d2.item_count = 0;                      expect(fb, "item_count = 0", run(b), TLSAN_E_BADARG);
  d2 = gd; d2.item_count = (1 << 30) + 1;          expect(fb, "item_count = 2^30 + 1", run(b), TLSAN_E_BADARG);
  tlsan_params p2 = gp; p2.item_emb = nullptr; b = gb; b.p = &p2;
  expect(fb, "item_emb NULL", run(b), TLSAN_E_BADARG);
  p2 = gp; p2.cate_emb = nullptr;                  expect(fb, "cate_emb NULL", run(b), TLSAN_E_BADARG);
  p2 = gp; p2.item_cate = nullptr;                 expect(fb, "item_cate NULL", run(b), TLSAN_E_BADARG);
  p2 = gp; p2.table_dtype = 2;                     expect(fb, "table_dtype = 2", run(b), TLSAN_E_BADARG);

  const char* ft = "tlsan_shortlist_topk";
  const size_t need = tlsan_shortlist_workspace_bytes(1000, 40, 128, 64);
  const Topk gt = {FAKE, 1000, 128, FAKE, 40, nullptr, FAKE, 1, 64, nullptr, nullptr, 1, 0, FAKE, FAKE, FAKE, need};
  Topk t = gt; t.vec = nullptr;                    expect(ft, "vec NULL", run(t), TLSAN_E_BADARG);
  t = gt; t.u_t = nullptr;                         expect(ft, "u_t NULL", run(t), TLSAN_E_BADARG);
  t = gt; t.item_b = nullptr;                      expect(ft, "item_b NULL", run(t), TLSAN_E_BADARG);
  t = gt; t.ids = nullptr;                         expect(ft, "ids NULL", run(t), TLSAN_E_BADARG);
  t = gt; t.approx = nullptr;                      expect(ft, "approx NULL", run(t), TLSAN_E_BADARG);
  t = gt; t.d = 96;                                expect(ft, "d = 96", run(t), TLSAN_E_UNSUPPORTED);
  t = gt; t.d = 512;                               expect(ft, "d = 512", run(t), TLSAN_E_UNSUPPORTED);
  t = gt; t.N = 15;                                expect(ft, "N = 15", run(t), TLSAN_E_BADARG);
  t = gt; t.N = 257;                               expect(ft, "N = 257", run(t), TLSAN_E_BADARG);
  t = gt; t.I = 0;                                 expect(ft, "I = 0", run(t), TLSAN_E_BADARG);
  t = gt; t.B = 0;                                 expect(ft, "B = 0", run(t), TLSAN_E_BADARG);
  t = gt; t.B = (1 << 24) + 1;                     expect(ft, "B = 2^24 + 1", run(t), TLSAN_E_BADARG);
  t = gt; t.xo = FAKE;                             expect(ft, "excl_off without excl_ids", run(t), TLSAN_E_BADARG);
  t = gt; t.xi = FAKE;                             expect(ft, "excl_ids without excl_off", run(t), TLSAN_E_BADARG);
  t = gt; t.ld = 0;                                expect(ft, "ld_itemb = 0", run(t), TLSAN_E_BADARG);
  t = gt; t.mul = 0;                               expect(ft, "id_mul = 0", run(t), TLSAN_E_BADARG);
  t = gt; t.add = -1;                              expect(ft, "id_add = -1", run(t), TLSAN_E_BADARG);
  t = gt; t.mul = 1 << 22;                         expect(ft, "ids past int32", run(t), TLSAN_E_BADARG);
  t = gt; t.ws = nullptr;                          expect(ft, "ws NULL", run(t), TLSAN_E_WORKSPACE);
  t = gt; t.ws_bytes = need - 1;                   expect(ft, "ws one byte short", run(t), TLSAN_E_WORKSPACE);
  t = gt; t.ws_bytes = 0;                          expect(ft, "no workspace", run(t), TLSAN_E_WORKSPACE);
  t = gt; t.I = 1 << 30; t.B = 1 << 24; t.N = 256; t.d = 256;
  expect(ft, "the largest call", run(t), TLSAN_E_UNSUPPORTED);

  const char* fs = "tlsan_shortlist_select";
  const Select gs = {FAKE, FAKE, FAKE, FAKE, nullptr, FAKE, 40, 128, 64, 10, FAKE, FAKE, FAKE};
  Select s = gs; s.sid = nullptr;                  expect(fs, "sl_ids NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.exact = nullptr;                       expect(fs, "sl_exact NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.approx = nullptr;                      expect(fs, "sl_approx NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.u_t = nullptr;                         expect(fs, "u_t NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.wmax = nullptr;                        expect(fs, "wmax NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.ids = nullptr;                         expect(fs, "ids NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.scores = nullptr;                      expect(fs, "scores NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.cert = nullptr;                        expect(fs, "certified NULL", run(s), TLSAN_E_BADARG);
  s = gs; s.d = 100;                               expect(fs, "d = 100", run(s), TLSAN_E_UNSUPPORTED);
  s = gs; s.N = 15;                                expect(fs, "N = 15", run(s), TLSAN_E_BADARG);
  s = gs; s.N = 257;                               expect(fs, "N = 257", run(s), TLSAN_E_BADARG);
  s = gs; s.K = 0;                                 expect(fs, "K = 0", run(s), TLSAN_E_BADARG);
  s = gs; s.K = 64;                                expect(fs, "K = N", run(s), TLSAN_E_BADARG);
  s = gs; s.K = 65;                                expect(fs, "K = N + 1", run(s), TLSAN_E_BADARG);
  s = gs; s.B = 0;                                 expect(fs, "B = 0", run(s), TLSAN_E_BADARG);
  s = gs; s.B = (1 << 24) + 1;                     expect(fs, "B = 2^24 + 1", run(s), TLSAN_E_BADARG);

  printf(bad ? "%d refusals WRONG\n" : "all refusals as specified\n", bad);
  return bad != 0;
}

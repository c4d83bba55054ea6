// The workspace sizes and the refusals of tlsan_shelves_workspace_bytes and tlsan_eval_shelves as a stand-alone host
// program, for a sanitizer run of the entry points' host side (tlsan_shelves.hip: argument checks and workspace carve-up)
// without Python and without a GPU: every call of tlsan_eval_shelves below must be refused before any launch, on fake
// pointers that are never dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_shelves.hip -x hip scripts/shelves_refusals.cpp -o shelves_refusals && ./shelves_refusals
// What tlsan_shelves.hip takes from the other units of the library this program brings itself: fail() and
// tlsan_last_error(), shape_of() and check_params() (tlsan_api.hip's checks, with the list of (d, heads) pairs written out).
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

int shape_of(const tlsan_dims* d, Shape* s) {
  if (!d) return fail(TLSAN_E_BADARG, "dims is NULL");
  if (d->num_heads <= 0 || d->d % d->num_heads) return fail(TLSAN_E_BADARG, "d %% num_heads != 0");
  if (d->d_item + d->d_cate != d->d) return fail(TLSAN_E_BADARG, "d_item + d_cate != d");
  if (d->user_count < 1 || d->item_count < 1 || d->cate_count < 1) return fail(TLSAN_E_BADARG, "empty table");
  const int pairs[6][2] = {{64, 4}, {64, 8}, {128, 4}, {128, 8}, {128, 16}, {256, 8}};
  for (const auto& pr : pairs)
    if (pr[0] == d->d && pr[1] == d->num_heads) {
      memset(s, 0, sizeof(*s));
      s->D = d->d;
      s->DH = d->d / d->num_heads;
      return TLSAN_OK;
    }
  return fail(TLSAN_E_UNSUPPORTED, "unsupported (hidden_units=%d, num_heads=%d)", d->d, d->num_heads);
}

int check_params(const tlsan_params* p) {
  if (!p || !p->item_emb || !p->item_b || !p->user_emb || !p->usert_emb || !p->cate_emb || !p->dense || !p->dense_KT ||
      !p->item_cate)
    return fail(TLSAN_E_BADARG, "NULL parameter pointer");
  return TLSAN_OK;
}

static void* const FAKE = (void*)0x1000;

struct Call {
  const tlsan_dims* d;
  const tlsan_params* p;
  const void* ut;
  int32_t B, S, m, min_items, rank_at;
  const void *off, *xid, *loff, *items;
  int32_t nlists, max_list;
  const void *so, *sl;
  int32_t nseg, nsmall;
  const void *bo, *bs;
  int32_t nbig, nbs;
  const void* skip;
  int32_t X, mul, add;
  void *cats, *ids, *scores, *ws;
  size_t ws_bytes;
};

static int run(const Call& c) {
  return tlsan_eval_shelves(c.d, c.p, (const float*)c.ut, c.B, c.S, c.m, c.min_items, c.rank_at, (const int32_t*)c.off,
                            (const int32_t*)c.xid, (const int32_t*)c.loff, (const int32_t*)c.items, c.nlists, c.max_list,
                            (const int32_t*)c.so, (const int32_t*)c.sl, c.nseg, c.nsmall, (const int32_t*)c.bo, (const int32_t*)c.bs,
                            c.nbig, c.nbs, (const int32_t*)c.skip, c.X, c.mul, c.add, (int32_t*)c.cats, (int32_t*)c.ids,
                            (float*)c.scores, c.ws, c.ws_bytes, nullptr);
}

static int bad = 0;
static void expect(const char* what, const Call& c, int code) {
  const int rc = run(c);
  const bool ok = rc == code && strstr(tlsan_last_error(), "tlsan_eval_shelves") != nullptr;
  printf("%-28s rc %d  \"%s\"  %s\n", what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
  bad += !ok;
}

static size_t size_of(const tlsan_dims* d, int32_t B, int32_t S, int32_t m, int32_t nseg, int32_t nbig, int32_t nbs) {
  return tlsan_shelves_workspace_bytes(d, B, S, m, nseg, nbig, nbs);
}

static void expect_size(const char* what, const tlsan_dims* d, int32_t B, int32_t S, int32_t m, int32_t nseg, int32_t nbig, int32_t nbs,
                        bool zero) {
  const size_t n = size_of(d, B, S, m, nseg, nbig, nbs);
  const bool ok = zero ? (n == 0 && strstr(tlsan_last_error(), "tlsan_shelves_workspace_bytes") != nullptr) : n > 0;
  printf("%-28s %zu bytes  %s\n", what, n, ok ? "ok" : "WRONG");
  bad += !ok;
}

static void expect_grows(const char* what, size_t small, size_t large) {
  const bool ok = small > 0 && large > small;
  printf("%-28s %zu < %zu  %s\n", what, small, large, ok ? "ok" : "WRONG");
  bad += !ok;
}

int main() {
  const tlsan_dims dims = {100, 200, 10, 128, 64, 64, 8, 10};
  tlsan_dims split = dims, pair = dims;
  split.d_cate = 32;
  pair.d = 96; pair.d_item = pair.d_cate = 48;
  tlsan_params p;
  memset(&p, 0, sizeof(p));
  p.item_emb = p.item_b = p.user_emb = p.usert_emb = p.cate_emb = p.dense = p.dense_KT = (float*)FAKE;
  p.item_cate = (const int32_t*)FAKE;
  tlsan_params hole = p;
  hole.item_cate = nullptr;

  expect_size("size: 3 segments, 2 big", &dims, 37, 4, 10, 3, 2, 5, false);
  expect_size("size: an empty index", &dims, 37, 4, 10, 0, 0, 0, false);
  expect_size("size: segments only", &dims, 37, 4, 10, 3, 0, 0, false);
  expect_size("size: big lists only", &dims, 37, 4, 10, 0, 2, 32, false);
  expect_size("size: the largest call", &dims, 1 << 24, 32, 8, 32767, 32767, 32767, false);
  expect_size("size: dims NULL", nullptr, 37, 4, 10, 3, 2, 5, true);
  expect_size("size: d_item + d_cate != d", &split, 37, 4, 10, 3, 2, 5, true);
  expect_size("size: d = 96", &pair, 37, 4, 10, 3, 2, 5, true);
  expect_size("size: B = 0", &dims, 0, 4, 10, 3, 2, 5, true);
  expect_size("size: B = 2^24 + 1", &dims, (1 << 24) + 1, 4, 10, 3, 2, 5, true);
  expect_size("size: S = 0", &dims, 37, 0, 10, 3, 2, 5, true);
  expect_size("size: S = 33", &dims, 37, 33, 7, 3, 2, 5, true);
  expect_size("size: m = 0", &dims, 37, 4, 0, 3, 2, 5, true);
  expect_size("size: m = 65", &dims, 37, 3, 65, 3, 2, 5, true);
  expect_size("size: S * m = 260", &dims, 37, 5, 52, 3, 2, 5, true);
  expect_size("size: nseg = -1", &dims, 37, 4, 10, -1, 2, 5, true);
  expect_size("size: nseg = 32768", &dims, 37, 4, 10, 32768, 2, 5, true);
  expect_size("size: nbig = -1", &dims, 37, 4, 10, 3, -1, 5, true);
  expect_size("size: nbs < nbig", &dims, 37, 4, 10, 3, 2, 1, true);
  expect_size("size: nbs > 16 nbig", &dims, 37, 4, 10, 3, 2, 33, true);
  expect_size("size: slices without a list", &dims, 37, 4, 10, 3, 0, 1, true);
  const size_t need = size_of(&dims, 37, 4, 10, 3, 2, 5);
  expect_grows("size grows with B", need, size_of(&dims, 38, 4, 10, 3, 2, 5));
  expect_grows("size grows with S", need, size_of(&dims, 37, 5, 10, 3, 2, 5));
  expect_grows("size grows with m", need, size_of(&dims, 37, 4, 11, 3, 2, 5));
  expect_grows("size grows with nseg", need, size_of(&dims, 37, 4, 10, 4, 2, 5));
  expect_grows("size grows with nbig", need, size_of(&dims, 37, 4, 10, 3, 3, 6));

  const Call good = {&dims, &p, FAKE, 37, 4, 10, 2, 1, nullptr, nullptr, FAKE, FAKE, 10, 50, FAKE, FAKE, 3, 8, FAKE, FAKE, 2, 5,
                     nullptr, 0, 1, 0, FAKE, FAKE, FAKE, FAKE, (size_t)1 << 40};
  Call c = good; c.d = nullptr;                  expect("dims NULL", c, TLSAN_E_BADARG);
  c = good; c.d = &split;                        expect("d_item + d_cate != d", c, TLSAN_E_BADARG);
  c = good; c.d = &pair;                         expect("d = 96", c, TLSAN_E_UNSUPPORTED);
  c = good; c.p = nullptr;                       expect("params NULL", c, TLSAN_E_BADARG);
  c = good; c.p = &hole;                         expect("item_cate NULL", c, TLSAN_E_BADARG);
  c = good; c.ut = nullptr;                      expect("u_t NULL", c, TLSAN_E_BADARG);
  c = good; c.cats = nullptr;                    expect("cats NULL", c, TLSAN_E_BADARG);
  c = good; c.ids = nullptr;                     expect("ids NULL", c, TLSAN_E_BADARG);
  c = good; c.scores = nullptr;                  expect("scores NULL", c, TLSAN_E_BADARG);
  c = good; c.B = 0;                             expect("B = 0", c, TLSAN_E_BADARG);
  c = good; c.B = -5;                            expect("B = -5", c, TLSAN_E_BADARG);
  c = good; c.S = 0;                             expect("S = 0", c, TLSAN_E_BADARG);
  c = good; c.S = 33; c.m = 7;                   expect("S = 33", c, TLSAN_E_BADARG);
  c = good; c.m = 0;                             expect("m = 0", c, TLSAN_E_BADARG);
  c = good; c.m = 65;                            expect("m = 65", c, TLSAN_E_BADARG);
  c = good; c.S = 5; c.m = 52;                   expect("S * m = 260", c, TLSAN_E_BADARG);
  c = good; c.min_items = 0;                     expect("min_items = 0", c, TLSAN_E_BADARG);
  c = good; c.min_items = 11;                    expect("min_items > m", c, TLSAN_E_BADARG);
  c = good; c.rank_at = -1;                      expect("rank_at = -1", c, TLSAN_E_BADARG);
  c = good; c.rank_at = 2;                       expect("rank_at = min_items", c, TLSAN_E_BADARG);
  c = good; c.nlists = 0;                        expect("nlists = 0", c, TLSAN_E_BADARG);
  c = good; c.nlists = (1 << 24) + 1;            expect("nlists = 2^24 + 1", c, TLSAN_E_BADARG);
  c = good; c.max_list = -1;                     expect("max_list = -1", c, TLSAN_E_BADARG);
  c = good; c.loff = nullptr;                    expect("list_off NULL", c, TLSAN_E_BADARG);
  c = good; c.items = nullptr;                   expect("list_items NULL", c, TLSAN_E_BADARG);
  c = good; c.so = nullptr;                      expect("seg_off NULL", c, TLSAN_E_BADARG);
  c = good; c.sl = nullptr;                      expect("seg_lists NULL", c, TLSAN_E_BADARG);
  c = good; c.bo = nullptr;                      expect("big_off NULL", c, TLSAN_E_BADARG);
  c = good; c.bs = nullptr;                      expect("big_slices NULL", c, TLSAN_E_BADARG);
  c = good; c.nseg = -1;                         expect("nseg = -1", c, TLSAN_E_BADARG);
  c = good; c.nseg = 32768;                      expect("nseg = 32768", c, TLSAN_E_BADARG);
  c = good; c.nsmall = -1;                       expect("nsmall = -1", c, TLSAN_E_BADARG);
  c = good; c.nsmall = 0;                        expect("segments without lists", c, TLSAN_E_BADARG);
  c = good; c.nbig = -1;                         expect("nbig = -1", c, TLSAN_E_BADARG);
  c = good; c.nbs = 1;                           expect("nbs < nbig", c, TLSAN_E_BADARG);
  c = good; c.nbs = 33;                          expect("nbs > 16 nbig", c, TLSAN_E_BADARG);
  c = good; c.skip = FAKE;                       expect("skip with X = 0", c, TLSAN_E_BADARG);
  c = good; c.X = 1;                             expect("X without skip", c, TLSAN_E_BADARG);
  c = good; c.skip = FAKE; c.X = 9;              expect("X = 9", c, TLSAN_E_BADARG);
  c = good; c.skip = FAKE; c.X = -1;             expect("X = -1", c, TLSAN_E_BADARG);
  c = good; c.off = FAKE;                        expect("excl_off alone", c, TLSAN_E_BADARG);
  c = good; c.xid = FAKE;                        expect("excl_ids alone", c, TLSAN_E_BADARG);
  c = good; c.mul = 0;                           expect("id_mul = 0", c, TLSAN_E_BADARG);
  c = good; c.add = -1;                          expect("id_add = -1", c, TLSAN_E_BADARG);
  c = good; c.mul = 1 << 30;                     expect("ids past int32", c, TLSAN_E_BADARG);
  c = good; c.ws = nullptr;                      expect("ws NULL", c, TLSAN_E_WORKSPACE);
  c = good; c.ws_bytes = need - 1;               expect("ws one byte short", c, TLSAN_E_WORKSPACE);
  c = good; c.ws_bytes = 0;                      expect("no workspace", c, TLSAN_E_WORKSPACE);
  c = good; c.B = 1 << 24; c.S = 32; c.m = 8; c.min_items = 8; c.rank_at = 7; c.nseg = c.nbig = c.nbs = 32767; c.ws_bytes = 1 << 20;
  expect("the largest call, 1 MiB", c, TLSAN_E_WORKSPACE);
  c = good; c.so = c.sl = nullptr; c.nseg = c.nsmall = 0; c.skip = FAKE; c.X = 8; c.off = c.xid = FAKE; c.ws_bytes = 0;
  expect("no segments, skip, excl", c, TLSAN_E_WORKSPACE);      // (all allowed: on to the workspace)
  c = good; c.bo = c.bs = nullptr; c.nbig = c.nbs = 0; c.ws_bytes = 0;
  expect("no big lists", c, TLSAN_E_WORKSPACE);
  printf(bad ? "%d refusals WRONG\n" : "all refusals as specified\n", bad);
  return bad != 0;
}

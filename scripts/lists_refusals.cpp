// The refusals of tlsan_lists_workspace_bytes, tlsan_eval_topk_lists and tlsan_similar_topk_lists as a stand-alone host
// program, for a sanitizer run of the entry points' host side (tlsan_lists.hip: argument checks and workspace carve-up)
// without Python and without a GPU: every call below must be refused before any launch, on fake pointers that are never
// dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_lists.hip -x hip scripts/lists_refusals.cpp -o lists_refusals && ./lists_refusals
// What tlsan_lists.hip takes from the other units of the library this program brings itself: fail() and
// tlsan_last_error(), shape_of() and check_params() (tlsan_api.hip's checks, with the list of (d, heads) pairs written out),
// and a stand-in for the merge's launcher, which no refused call reaches (it aborts if one does).
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

hipError_t tlsan_launch_topk_merge(const int32_t*, const float*, int, int, int, int32_t*, float*, hipStream_t) {
  printf("a refused call reached a launcher\n");
  abort();
}

static void* const FAKE = (void*)0x1000;

struct Call {
  const tlsan_dims* d;
  const tlsan_params* p;
  const void *rows, *qinv, *qids;      // u_t / qvec; the similar form's qinv and qids
  int32_t B, K, metric;
  const void *off, *xid, *loff, *items;
  int32_t nlists, max_list;
  const void* probes;
  int32_t P, mul, add;
  void *ids, *scores, *ws;
  size_t ws_bytes;
};

static int run_topk(const Call& c) {
  return tlsan_eval_topk_lists(c.d, c.p, (const float*)c.rows, c.B, c.K, (const int32_t*)c.off, (const int32_t*)c.xid,
                               (const int32_t*)c.loff, (const int32_t*)c.items, c.nlists, c.max_list, (const int32_t*)c.probes,
                               c.P, c.mul, c.add, (int32_t*)c.ids, (float*)c.scores, c.ws, c.ws_bytes, nullptr);
}

static int run_similar(const Call& c) {
  return tlsan_similar_topk_lists(c.d, c.p, (const float*)c.rows, (const float*)c.qinv, (const int32_t*)c.qids, c.B, c.K,
                                  c.metric, (const int32_t*)c.off, (const int32_t*)c.xid, (const int32_t*)c.loff,
                                  (const int32_t*)c.items, c.nlists, c.max_list, (const int32_t*)c.probes, c.P, c.mul, c.add,
                                  (int32_t*)c.ids, (float*)c.scores, c.ws, c.ws_bytes, nullptr);
}

static int bad = 0;
static void expect(const char* what, const Call& c, int code) {
  const struct { int (*run)(const Call&); const char* name; } fns[2] = {{run_topk, "tlsan_eval_topk_lists"},
                                                                        {run_similar, "tlsan_similar_topk_lists"}};
  for (const auto& f : fns) {
    const int rc = f.run(c);
    const bool ok = rc == code && strstr(tlsan_last_error(), f.name) != nullptr;
    printf("%-28s rc %d  \"%s\"  %s\n", what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
    bad += !ok;
  }
}

static void expect_size(const char* what, const tlsan_dims* d, int32_t B, int32_t P, int32_t K, int32_t nlists, int32_t max_list,
                        bool zero) {
  const size_t n = tlsan_lists_workspace_bytes(d, B, P, K, nlists, max_list);
  const bool ok = zero ? (n == 0 && strstr(tlsan_last_error(), "tlsan_lists_workspace_bytes") != nullptr) : n > 0;
  printf("%-28s %zu bytes  %s\n", what, n, ok ? "ok" : "WRONG");
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

  expect_size("size: 10 lists of <= 50", &dims, 4, 2, 16, 10, 50, false);
  expect_size("size: an empty index", &dims, 4, 2, 16, 10, 0, false);
  expect_size("size: the largest call", &dims, 1 << 24, 8, 256, 1 << 24, 1 << 30, false);
  expect_size("size: dims NULL", nullptr, 4, 2, 16, 10, 50, true);
  expect_size("size: d_item + d_cate != d", &split, 4, 2, 16, 10, 50, true);
  expect_size("size: d = 96", &pair, 4, 2, 16, 10, 50, true);
  expect_size("size: B = 0", &dims, 0, 2, 16, 10, 50, true);
  expect_size("size: B = 2^24 + 1", &dims, (1 << 24) + 1, 2, 16, 10, 50, true);
  expect_size("size: P = 0", &dims, 4, 0, 16, 10, 50, true);
  expect_size("size: P = 9", &dims, 4, 9, 16, 10, 50, true);
  expect_size("size: K = 0", &dims, 4, 2, 0, 10, 50, true);
  expect_size("size: K = 257", &dims, 4, 2, 257, 10, 50, true);
  expect_size("size: nlists = 0", &dims, 4, 2, 16, 0, 50, true);
  expect_size("size: max_list = -1", &dims, 4, 2, 16, 10, -1, true);
  const size_t need = tlsan_lists_workspace_bytes(&dims, 4, 2, 16, 10, 50);

  const Call good = {&dims, &p, FAKE, FAKE, FAKE, 4, 16, TLSAN_SIM_COSINE, nullptr, nullptr, FAKE, FAKE, 10, 50, FAKE, 2, 1, 0,
                     FAKE, FAKE, FAKE, (size_t)1 << 40};
  Call c = good; c.d = nullptr;                  expect("dims NULL", c, TLSAN_E_BADARG);
  c = good; c.d = &split;                        expect("d_item + d_cate != d", c, TLSAN_E_BADARG);
  c = good; c.d = &pair;                         expect("d = 96", c, TLSAN_E_UNSUPPORTED);
  c = good; c.p = nullptr;                       expect("params NULL", c, TLSAN_E_BADARG);
  c = good; c.p = &hole;                         expect("item_cate NULL", c, TLSAN_E_BADARG);
  c = good; c.rows = nullptr;                    expect("u_t / qvec NULL", c, TLSAN_E_BADARG);
  c = good; c.ids = nullptr;                     expect("ids NULL", c, TLSAN_E_BADARG);
  c = good; c.scores = nullptr;                  expect("scores NULL", c, TLSAN_E_BADARG);
  c = good; c.B = 0;                             expect("B / Q = 0", c, TLSAN_E_BADARG);
  c = good; c.B = -5;                            expect("B / Q = -5", c, TLSAN_E_BADARG);
  c = good; c.K = 0;                             expect("K = 0", c, TLSAN_E_BADARG);
  c = good; c.K = 257;                           expect("K = 257", c, TLSAN_E_BADARG);
  c = good; c.P = 0;                             expect("P = 0", c, TLSAN_E_BADARG);
  c = good; c.P = 9;                             expect("P = 9", c, TLSAN_E_BADARG);
  c = good; c.nlists = 0;                        expect("nlists = 0", c, TLSAN_E_BADARG);
  c = good; c.max_list = -1;                     expect("max_list = -1", c, TLSAN_E_BADARG);
  c = good; c.loff = nullptr;                    expect("list_off NULL", c, TLSAN_E_BADARG);
  c = good; c.items = nullptr;                   expect("list_items NULL", c, TLSAN_E_BADARG);
  c = good; c.probes = nullptr;                  expect("row_lists NULL", c, TLSAN_E_BADARG);
  c = good; c.off = FAKE;                        expect("excl_off alone", c, TLSAN_E_BADARG);
  c = good; c.xid = FAKE;                        expect("excl_ids alone", c, TLSAN_E_BADARG);
  c = good; c.mul = 0;                           expect("id_mul = 0", c, TLSAN_E_BADARG);
  c = good; c.add = -1;                          expect("id_add = -1", c, TLSAN_E_BADARG);
  c = good; c.mul = 1 << 30;                     expect("ids past int32", c, TLSAN_E_BADARG);
  c = good; c.ws = nullptr;                      expect("ws NULL", c, TLSAN_E_WORKSPACE);
  c = good; c.ws_bytes = need - 1;               expect("ws one byte short", c, TLSAN_E_WORKSPACE);
  c = good; c.ws_bytes = 0;                      expect("no workspace", c, TLSAN_E_WORKSPACE);
  c = good; c.B = 1 << 24; c.P = 8; c.K = 256; c.nlists = 1 << 24; c.max_list = 1 << 30; c.ws_bytes = 1 << 20;
  expect("the largest call, 1 MiB", c, TLSAN_E_WORKSPACE);
  c = good; c.metric = 2;
  {
    const int rc = run_similar(c);
    const bool ok = rc == TLSAN_E_BADARG && strstr(tlsan_last_error(), "tlsan_similar_topk_lists: metric") != nullptr;
    printf("%-28s rc %d  \"%s\"  %s\n", "metric = 2", rc, tlsan_last_error(), ok ? "ok" : "WRONG");
    bad += !ok;
  }
  printf(bad ? "%d refusals WRONG\n" : "all refusals as specified\n", bad);
  return bad != 0;
}

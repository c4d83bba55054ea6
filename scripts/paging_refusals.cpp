// The refusals of tlsan_eval_topk_scoped_after, tlsan_eval_topk_lists_after and tlsan_dense_topk_after as a stand-alone host
// program, for a sanitizer run of the entry points' host side (tlsan_after.hip with the checks and carve-ups of
// tlsan_scope_host.h, tlsan_lists_host.h and tlsan_dense_host.h) without Python and without a GPU: every call below must be
// refused before any launch, on fake pointers that are never dereferenced.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itlsan_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         tlsan_amd/csrc/tlsan_after.hip -x hip scripts/paging_refusals.cpp -o paging_refusals && ./paging_refusals
// What tlsan_after.hip takes from the other units of the library this program brings itself: fail() and
// tlsan_last_error(), shape_of() and check_params() (tlsan_api.hip's checks, with the list of (d, heads) pairs written out),
// and stand-ins for the grouping's and the merge's launchers, which no refused call reaches (they abort if one does).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tlsan_dense_host.h"
#include "tlsan_lists_host.h"

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

hipError_t tlsan_launch_lists_group(const ListsArgs&, hipStream_t) {
  printf("a refused call reached a launcher\n");
  abort();
}

static void* const FAKE = (void*)0x1000;

struct Call {
  const tlsan_dims* d;
  const tlsan_params* p;
  const void* rows;
  int32_t B, K;
  const void *off, *xid;
  const void* sub;                     // the scoped call's scope
  int32_t nsub;
  const void* cate;
  const void *loff, *items;            // the indexed call's index
  int32_t nlists, max_list;
  const void* probes;
  int32_t P, mul, add;
  void *ids, *scores, *ws;
  size_t ws_bytes;
  const void *boost, *weight;
  const void *aid, *asc;               // the cursors
  const void* x;                       // the dense call's matrix, its N and d
  int32_t N, dd;
};

static int run_scoped(const Call& c) {
  return tlsan_eval_topk_scoped_after(c.d, c.p, (const float*)c.rows, c.B, c.K, (const int32_t*)c.off, (const int32_t*)c.xid,
                                      (const int32_t*)c.sub, c.nsub, (const int32_t*)c.cate, c.mul, c.add, (int32_t*)c.ids,
                                      (float*)c.scores, c.ws, c.ws_bytes, nullptr, (const float*)c.boost, (const float*)c.weight,
                                      (const int32_t*)c.aid, (const float*)c.asc);
}

static int run_lists(const Call& c) {
  return tlsan_eval_topk_lists_after(c.d, c.p, (const float*)c.rows, c.B, c.K, (const int32_t*)c.off, (const int32_t*)c.xid,
                                     (const int32_t*)c.loff, (const int32_t*)c.items, c.nlists, c.max_list,
                                     (const int32_t*)c.probes, c.P, c.mul, c.add, (int32_t*)c.ids, (float*)c.scores, c.ws,
                                     c.ws_bytes, nullptr, (const float*)c.boost, (const float*)c.weight, (const int32_t*)c.aid,
                                     (const float*)c.asc);
}

// (the dense call: rows are the queries, B their number; no table, no boost)
static int run_dense(const Call& c) {
  return tlsan_dense_topk_after((const float*)c.rows, c.B, c.dd, (const float*)c.x, c.N, nullptr, nullptr, (const int32_t*)c.off,
                                (const int32_t*)c.xid, c.add, c.K, (int32_t*)c.ids, (float*)c.scores, c.ws, c.ws_bytes, nullptr,
                                (const int32_t*)c.aid, (const float*)c.asc);
}

static int bad = 0, made = 0;
enum { SCOPED = 1, LISTS = 2, TABLE = 3, DENSE = 4, ALL = 7 };
static void expect(const char* what, const Call& c, int code, int which, const char* word = nullptr) {
  const struct { int bit; int (*run)(const Call&); const char* name; } fns[3] = {{SCOPED, run_scoped, "tlsan_eval_topk_scoped_after"},
                                                                                 {LISTS, run_lists, "tlsan_eval_topk_lists_after"},
                                                                                 {DENSE, run_dense, "tlsan_dense_topk_after"}};
  for (const auto& f : fns) {
    if (!(which & f.bit)) continue;
    // (the table calls: without a boost, with one, with one and row weights -- none changes a refusal)
    for (int form = 0; form < (f.bit == DENSE ? 1 : 3); ++form) {
      Call cc = c;
      if (f.bit != DENSE && !word) {
        cc.boost = form ? FAKE : nullptr;
        cc.weight = form == 2 ? FAKE : nullptr;
      } else if (form) {
        continue;
      }
      const int rc = f.run(cc);
      const bool ok = rc == code && strstr(tlsan_last_error(), f.name) != nullptr && (!word || strstr(tlsan_last_error(), word) != nullptr);
      if (!form || !ok) printf("%-28s rc %d  \"%s\"  %s\n", what, rc, tlsan_last_error(), ok ? "ok" : "WRONG");
      bad += !ok;
      ++made;
    }
  }
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

  ScopeWs sw;
  carve_scope(&dims, 4, 16, 50, nullptr, &sw);
  ListsWs lw;
  carve_lists(&dims, 4, 2, 16, 10, 50, nullptr, &lw);
  DenseWs dw;
  carve_dense(4, 1000, 16, nullptr, &dw);

  const Call good = {&dims, &p, FAKE, 4, 16, nullptr, nullptr, FAKE, 50, FAKE, FAKE, FAKE, 10, 50, FAKE, 2, 1, 0,
                     FAKE, FAKE, FAKE, (size_t)1 << 40, FAKE, nullptr, FAKE, FAKE, FAKE, 1000, 128};
  // the cursor, and the weight that needs a boost
  Call c = good; c.aid = nullptr;                expect("after_ids NULL", c, TLSAN_E_BADARG, ALL, "without a cursor");
  c = good; c.asc = nullptr;                     expect("after_scores NULL", c, TLSAN_E_BADARG, ALL, "without a cursor");
  c = good; c.aid = c.asc = nullptr; c.boost = nullptr;
  expect("no cursor, no boost", c, TLSAN_E_BADARG, ALL, "without a cursor");
  c = good; c.aid = nullptr; c.ws_bytes = 0;     expect("after_ids NULL, no workspace", c, TLSAN_E_BADARG, TABLE, "without a cursor");
  c = good; c.boost = nullptr; c.weight = FAKE;  expect("row_weight without boost", c, TLSAN_E_BADARG, TABLE, "row_weight");
  // what the twins refuse
  c = good; c.d = nullptr;                       expect("dims NULL", c, TLSAN_E_BADARG, TABLE);
  c = good; c.d = &split;                        expect("d_item + d_cate != d", c, TLSAN_E_BADARG, TABLE);
  c = good; c.d = &pair;                         expect("d = 96", c, TLSAN_E_UNSUPPORTED, TABLE);
  c = good; c.p = nullptr;                       expect("params NULL", c, TLSAN_E_BADARG, TABLE);
  c = good; c.p = &hole;                         expect("item_cate NULL", c, TLSAN_E_BADARG, TABLE);
  c = good; c.rows = nullptr;                    expect("u_t / q NULL", c, TLSAN_E_BADARG, ALL);
  c = good; c.ids = nullptr;                     expect("ids NULL", c, TLSAN_E_BADARG, ALL);
  c = good; c.scores = nullptr;                  expect("scores NULL", c, TLSAN_E_BADARG, ALL);
  c = good; c.B = 0;                             expect("B / Q = 0", c, TLSAN_E_BADARG, ALL);
  c = good; c.B = -5;                            expect("B / Q = -5", c, TLSAN_E_BADARG, ALL);
  c = good; c.K = 0;                             expect("K = 0", c, TLSAN_E_BADARG, ALL);
  c = good; c.K = 257;                           expect("K = 257", c, TLSAN_E_BADARG, ALL);
  c = good; c.off = FAKE;                        expect("excl_off alone", c, TLSAN_E_BADARG, ALL);
  c = good; c.xid = FAKE;                        expect("excl_ids alone", c, TLSAN_E_BADARG, ALL);
  c = good; c.mul = 0;                           expect("id_mul = 0", c, TLSAN_E_BADARG, TABLE);
  c = good; c.add = -1;                          expect("id_add = -1", c, TLSAN_E_BADARG, ALL);
  c = good; c.mul = 1 << 30;                     expect("ids past int32", c, TLSAN_E_BADARG, TABLE);
  c = good; c.ws = nullptr;                      expect("ws NULL", c, TLSAN_E_WORKSPACE, ALL);
  c = good; c.ws_bytes = 0;                      expect("no workspace", c, TLSAN_E_WORKSPACE, ALL);
  c = good; c.ws_bytes = sw.bytes - 1;           expect("ws one byte short", c, TLSAN_E_WORKSPACE, SCOPED);
  c = good; c.ws_bytes = lw.bytes - 1;           expect("ws one byte short", c, TLSAN_E_WORKSPACE, LISTS);
  c = good; c.ws_bytes = dw.bytes - 1;           expect("ws one byte short", c, TLSAN_E_WORKSPACE, DENSE);
  // the scope
  c = good; c.sub = nullptr; c.nsub = 0;         expect("sub NULL, nsub = 0", c, TLSAN_E_BADARG, SCOPED);
  c = good; c.sub = nullptr; c.nsub = 7;         expect("sub NULL, nsub = 7", c, TLSAN_E_BADARG, SCOPED);
  c = good; c.nsub = -1;                         expect("sub given, nsub = -1", c, TLSAN_E_BADARG, SCOPED);
  c = good; c.nsub = 201;                        expect("nsub past the table", c, TLSAN_E_BADARG, SCOPED);
  c = good; c.sub = nullptr; c.nsub = -1; c.ws_bytes = 0;
  expect("the whole table, no ws", c, TLSAN_E_WORKSPACE, SCOPED);
  // the index
  c = good; c.P = 0;                             expect("P = 0", c, TLSAN_E_BADARG, LISTS);
  c = good; c.P = 9;                             expect("P = 9", c, TLSAN_E_BADARG, LISTS);
  c = good; c.nlists = 0;                        expect("nlists = 0", c, TLSAN_E_BADARG, LISTS);
  c = good; c.nlists = (1 << 24) + 1;            expect("nlists = 2^24 + 1", c, TLSAN_E_BADARG, LISTS);
  c = good; c.B = (1 << 24) + 1;                 expect("B / Q = 2^24 + 1", c, TLSAN_E_BADARG, LISTS | DENSE);
  c = good; c.max_list = -1;                     expect("max_list = -1", c, TLSAN_E_BADARG, LISTS);
  c = good; c.loff = nullptr;                    expect("list_off NULL", c, TLSAN_E_BADARG, LISTS);
  c = good; c.items = nullptr;                   expect("list_items NULL", c, TLSAN_E_BADARG, LISTS);
  c = good; c.probes = nullptr;                  expect("row_lists NULL", c, TLSAN_E_BADARG, LISTS);
  c = good; c.B = 1 << 24; c.P = 8; c.K = 256; c.nlists = 1 << 24; c.max_list = 1 << 30; c.ws_bytes = 1 << 20;
  expect("the largest call, 1 MiB", c, TLSAN_E_WORKSPACE, LISTS);
  // the dense matrix
  c = good; c.x = nullptr;                       expect("x NULL", c, TLSAN_E_BADARG, DENSE);
  c = good; c.dd = 96;                           expect("d = 96", c, TLSAN_E_UNSUPPORTED, DENSE);
  c = good; c.N = 0;                             expect("N = 0", c, TLSAN_E_BADARG, DENSE);
  c = good; c.N = (1 << 30) + 1;                 expect("N = 2^30 + 1", c, TLSAN_E_BADARG, DENSE);
  c = good; c.add = (1LL << 31) - 10;            expect("row ids past int32", c, TLSAN_E_BADARG, DENSE);
  c = good; c.B = 1 << 24; c.N = 1 << 30; c.K = 256; c.ws_bytes = 1 << 20;
  expect("the largest call, 1 MiB", c, TLSAN_E_WORKSPACE, DENSE);
  if (bad) printf("%d of %d refusals WRONG\n", bad, made);
  else printf("all %d refusals as specified\n", made);
  return bad != 0;
}

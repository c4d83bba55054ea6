// tlsan_after.h -- list cursors: the scoped lists (tlsan_scope.h), the indexed lists (tlsan_lists.h) and the dense lists
// (tlsan_dense.h) continued behind a position of their own order.  A row's cursor is a pair (after_id, after_score):
//   after_id >= 0                  the row selects item g only when topk_key(s'(b, g), g) < topk_key(after_score, after_id),
//                                  s' the score the call returns (the model's, or the boosted one: the boost is inside)
//   after_id == TLSAN_AFTER_START  no cursor: the row is the call's without one, ids and bits
//   any other negative id          the row is exhausted: nothing is selected, its page is -1 / -inf
// Eligibility, order, padding and the score bits are the call's: the page is the K best of what the same call without a
// cursor ranks strictly behind the cursor, so pages chained by their last entries tile the exact ranking.  The cursor is
// a position in the order, not an item: it need not be in the table, the scope or eligible; its zero's sign and its NaN
// payload do not matter, because tlsan_topk.h's key drops both.
// The cursor becomes one 64-bit CAP per row: ~0 for START, 0 for exhausted, else the cursor's key.  A real key is neither:
// its high word is 1 for a NaN, ~u in 0x007fffff (-inf) .. 0x7fffffff for a negative float u and u | 0x80000000 in
// 0x80000000 .. 0xff800000 (+inf) for the others -- never 0 and never 0xffffffff.  So `key < cap` holds for every item at
// START and for none on an exhausted row, without a branch of their own.
// Where the cap lives: 16 rows x 8 bytes of LDS beside TopkSmem, written in the scan's prologue (the policy's row(), in
// front of the scan's first barrier) and read in may().  The scans are not touched and carry no new register from round
// to round: k_boost_scoped_topk<256, ...> already sits at the register file's edge (profiles/boost.md), and four more
// 64-bit values per lane would spill there.  The four lanes' reads are LDS broadcasts (16 lanes share an address).
// The boost is optional in the one wrapper: a NULL boost is t = 0 with its load skipped behind a uniform branch, as a NULL
// row_weight is 1; fl(s + 0) keeps the key (-0 -> +0 is canonicalised anyway, NaN stays NaN), so one kernel serves both.
#pragma once
#include "tlsan_boost.h"
#include "tlsan_dense.h"

#define AFTER_START (-2)   // TLSAN_AFTER_START (include/tlsan.h)

struct AfterArgs {
  const int32_t* ids;     // [B] the cursors' ids
  const float* scores;    // [B] the cursors' scores
};

struct AfterScopedArgs { ScopedTopkArgs s; BoostArgs b; AfterArgs c; };
struct AfterListsArgs { ListsTopkArgs l; BoostArgs b; AfterArgs c; };
struct AfterDenseArgs { DenseTopkArgs d; AfterArgs c; };

__device__ __forceinline__ topk_key_t after_cap(int id, float score) {
  return id >= 0 ? topk_key(score, id) : (id == AFTER_START ? ~0ull : 0ull);
}

// Boosted<Base> (tlsan_boost.h) with the boost optional: NULL is t = 0, its load skipped (uniform).
template <class Base>
struct MaybeBoosted {
  Base base;
  const BoostArgs& b;
  const int id_mul, id_add;
  float w[4], t;
  template <class Args>
  __device__ __forceinline__ MaybeBoosted(const Args& args, const BoostArgs& b_, const EvalArgs& e)
      : base(args), b(b_), id_mul(e.id_mul), id_add(e.id_add), t(0.0f) {}
  __device__ __forceinline__ bool row(int i, int u) {
    const bool ok = base.row(i, u);          // (false for a row past B: its weight is not read)
    w[i] = (ok && b.row_weight) ? b.row_weight[u] : 1.0f;
    return ok;
  }
  __device__ __forceinline__ void col(const f32x4& tile, int item) {
    base.col(tile, item);
    if (b.boost) t = b.boost[(size_t)(item * id_mul + id_add)];   // (item is a table row: a position outside the table reads item 0)
  }
  __device__ __forceinline__ float score(int i) const {
#pragma clang fp contract(off)
    const float s = base.score(i);
    const float wt = w[i] * t;
    return s + wt;
  }
  __device__ __forceinline__ bool may(int i, int gn) const { return base.may(i, gn); }
};

// The cursor around a score policy: row() turns row u's cursor into its cap in LDS slot 4 q + i (the slot both scans give
// the lane's row i), may() adds `key < cap` to the base's test.  The key is formed from score(i) as the scan forms it: the
// same expression on the same operands, one value after inlining.
template <class Base>
struct After {
  Base base;
  const AfterArgs& c;
  topk_key_t* cap;        // LDS [16]
  template <class... A>
  __device__ __forceinline__ After(const AfterArgs& c_, topk_key_t* cap_, const A&... a) : base(a...), c(c_), cap(cap_) {}
  __device__ __forceinline__ bool row(int i, int u) {
    const bool ok = base.row(i, u);          // (false for a row past B: its cursor is not read, its cap is 0)
    const topk_key_t k = ok ? after_cap(c.ids[u], c.scores[u]) : 0ull;
    if ((threadIdx.x & 15) == 0) cap[4 * ((threadIdx.x >> 4) & 3) + i] = k;   // (the four wavefronts write the same value)
    return ok;
  }
  __device__ __forceinline__ void col(const f32x4& tile, int item) { base.col(tile, item); }
  __device__ __forceinline__ float score(int i) const { return base.score(i); }
  __device__ __forceinline__ bool may(int i, int gn) const {
    return base.may(i, gn) && topk_key(base.score(i), gn) < cap[4 * ((threadIdx.x >> 4) & 3) + i];
  }
};

// Workgroups per CU asked of the compiler: the twins' 2, and 3 for the three instantiations that under the twins' bound land
// one to four registers above the 168 VGPRs three workgroups a CU need, where their twins land below it (the cap's reads
// cost a register or two at the wrong side of that step): the scoped kernel at d = 64 with the short kept lists, the dense
// one at d = 128, KP = 64.  The bound makes the allocator stay under the step; none of them spills (profiles/paging.md).
#define AFTER_WG_SCOPED(D, KP) ((D) == 64 && (KP) <= 64 ? 3 : 2)
#define AFTER_WG_DENSE(D, KP) ((D) == 128 && (KP) == 64 ? 3 : 2)

// grid (ceil(B/16), slices of the scope's count): k_scoped_topk's
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, AFTER_WG_SCOPED(D, KP)) void k_after_scoped_topk(AfterScopedArgs aa) {
  __shared__ TopkSmem<KP, BUF> sm;
  __shared__ topk_key_t cap[16];
  After<MaybeBoosted<ScopedScore>> pol(aa.c, cap, aa.s, aa.b, aa.s.t.e);
  const ScopeMap map(aa.s.s, aa.s.t.e);
  topk_scan<D, KP, BUF, false>(sm, aa.s.t, pol, map);
}

// grid (groups bound, slices): k_lists_topk's
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_after_lists_topk(AfterListsArgs aa) {
  __shared__ TopkSmem<KP, BUF> sm;
  __shared__ topk_key_t cap[16];
  After<MaybeBoosted<ListScore>> pol(aa.c, cap, aa.l, aa.b, aa.l.t.e);
  lists_scan<D, KP, BUF>(sm, aa.l.t, aa.l.l, pol);
}

// grid (ceil(Q / 16), slices): k_dense_topk's
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, AFTER_WG_DENSE(D, KP)) void k_after_dense_topk(AfterDenseArgs aa) {
  __shared__ TopkSmem<KP, BUF> sm;
  __shared__ topk_key_t cap[16];
  After<DenseScore> pol(aa.c, cap, aa.d);
  topk_scan<D, KP, BUF, true>(sm, aa.d.t, pol, AllItems());
}

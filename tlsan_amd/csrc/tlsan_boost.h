// tlsan_boost.h -- per-item score adjustments inside the selection: the scoped lists (tlsan_scope.h) and the indexed lists
// (tlsan_lists.h) with one term added to the model's score before it meets the row's threshold,
//   s'(b, g) = fl(s(b, g) + t),   t = boost[g]                     without row weights
//                                 t = fl(row_weight[b] * boost[g])  with them
// g the column's GLOBAL id (local * id_mul + id_add), in fp32 with separate roundings (no FMA: contracted, s' would differ in
// the last bit from the sum a caller forms from the returned raw score, as k_eval_topk's two roundings would).  Selection,
// thresholds, the merge of slices and the order act on s' by tlsan_topk.h's key: higher first, equal -> lower global id,
// +0.0 == -0.0 (returned as +0.0), NaN last.  boost[g] = -inf gives s' = -inf, a valid score behind every finite one, not
// an exclusion; 0 * inf = NaN ranks last.  A boost of +0.0 gives the unboosted lists, ids and bits (s + 0 = s; a zero's sign
// is not in the key).
// The adjustment is a score policy around the base policy (ScopedScore, ListScore) on the scans as they stand: topk_scan
// and lists_scan are not touched.  col() loads boost[g] beside the base's own per-item loads (item_b, item_cate), all
// addressed by the column's item, which the scan knows before the tile's table loads: 4 bytes per column and one more load
// in a batch that is already in flight, not a dependent trip of its own.  row() loads the row's weight once, beside the
// exclusion offsets.  Without weights the weight is 1 and the product is exact (fl(1 * x) = x, NaN stays NaN), so there is
// one kernel per (D, KP, BUF) and not two.
#pragma once
#include "tlsan_lists.h"
#include "tlsan_scope.h"

struct BoostArgs {
  const float* boost;        // [every global id the id mapping can produce]
  const float* row_weight;   // [B] or NULL: 1
};

struct BoostedScopedArgs { ScopedTopkArgs s; BoostArgs b; };
struct BoostedListsArgs { ListsTopkArgs l; BoostArgs b; };

// (tlsan_after.h's MaybeBoosted<Base> is this policy with the boost optional, a text of its own so that the kernels here keep
//  their code: a change to row(), col() or score() goes into both.)
template <class Base>
struct Boosted {
  Base base;
  const BoostArgs& b;
  const int id_mul, id_add;
  float w[4], t;
  template <class Args>
  __device__ __forceinline__ Boosted(const Args& args, const BoostArgs& b_, const EvalArgs& e)
      : base(args), b(b_), id_mul(e.id_mul), id_add(e.id_add) {}
  __device__ __forceinline__ bool row(int i, int u) {
    const bool ok = base.row(i, u);          // (false for a row past B: its weight is not read)
    w[i] = (ok && b.row_weight) ? b.row_weight[u] : 1.0f;
    return ok;
  }
  __device__ __forceinline__ void col(const f32x4& tile, int item) {
    base.col(tile, item);
    t = b.boost[(size_t)(item * id_mul + id_add)];   // (item is a table row: a position outside the table reads item 0)
  }
  __device__ __forceinline__ float score(int i) const {
#pragma clang fp contract(off)
    const float s = base.score(i);
    const float wt = w[i] * t;
    return s + wt;
  }
  __device__ __forceinline__ bool may(int i, int gn) const { return base.may(i, gn); }
};

// grid (ceil(B/16), slices of the scope's count): k_scoped_topk's
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_boost_scoped_topk(BoostedScopedArgs ba) {
  __shared__ TopkSmem<KP, BUF> sm;
  Boosted<ScopedScore> pol(ba.s, ba.b, ba.s.t.e);
  const ScopeMap map(ba.s.s, ba.s.t.e);
  topk_scan<D, KP, BUF, false>(sm, ba.s.t, pol, map);
}

// grid (groups bound, slices): k_lists_topk's
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_boost_lists_topk(BoostedListsArgs ba) {
  __shared__ TopkSmem<KP, BUF> sm;
  Boosted<ListScore> pol(ba.l, ba.b, ba.l.t.e);
  lists_scan<D, KP, BUF>(sm, ba.l.t, ba.l.l, pol);
}

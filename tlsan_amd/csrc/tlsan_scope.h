// tlsan_scope.h -- scoped lists: the K best items of a SUBSET of a table's items, with an optional category wanted per
// row.  The selection is tlsan_topk.h's (keys, order, TopkSmem, topk_offer, topk_reselect, topk_finish, TOPK_DISPATCH, the
// exclusion lists) on topk_scan, whose item-mapping hook says which local item a scan position stands for:
//   sub == NULL   position n is local item n, count = I (what k_similar_topk runs: AllItems)
//   sub != NULL   position n is local item sub[n], count = nsub: the work is that of nsub items, not of I
// The global id of a column is local * id_mul + id_add either way.  sub is a caller's list: ascending, distinct local
// indices in [0, I).  An index outside [0, I) is never dereferenced as a table row: the column reads item 0 in its place
// and is never selected (ScopeMap::holds).  Repeats are not checked: a repeated index can appear twice in a list.
// A round's sub[n] are loaded a round ahead of the tiles that need them (ScopeMap::loaded), off the critical path of the
// tile's table loads, and looked at only when their round comes: one dword per column per round.
// Scores: the gather form only (score_tile through all_emb4); no dense [I, D] matrix is built for a scope.  A (row, item)
// score depends on neither the item's column nor its tile, so it equals k_eval_topk's, k_eval_label's and k_score_cand's
// (ScopedScore: eval_score, two roundings) and k_similar_topk's (ScopedSim: SimScore's products) bit for bit.
// The loop itself is topk_scan's, and k_eval_topk keeps a text of its own (tlsan_topk.h says why): a fix to the scan's
// prologue, tile loop or offer loop goes into both.
#pragma once
#include "tlsan_similar.h"

struct ScopeArgs {
  const int32_t* sub;        // [nsub] local item indices, ascending and distinct, or NULL: every item
  int32_t nsub;
  const int32_t* row_cate;   // [B] the category row b wants (< 0: any), or NULL: none
};

struct ScopedTopkArgs { TopkArgs t; ScopeArgs s; };
struct ScopedSimArgs { SimArgs m; ScopeArgs s; };

// topk_scan's item mapping of a scope
struct ScopeMap {
  static constexpr bool loaded = true;
  const int32_t* sub;
  const int nsub, I;
  __device__ __forceinline__ ScopeMap(const ScopeArgs& s, const EvalArgs& a) : sub(s.sub), nsub(s.nsub), I(a.I) {}
  __device__ __forceinline__ int count(const EvalArgs& a) const { return sub ? nsub : a.I; }
  __device__ __forceinline__ int local(int n) const { return sub ? sub[n] : n; }      // (as listed: holds() looks at it)
  __device__ __forceinline__ bool holds(int loc) const { return (unsigned)loc < (unsigned)I; }
};

// The category test of a scoped policy: row i wants want[i] (< 0: any); the column's category is read once, in col.
struct ScopeCate {
  const int32_t* row_cate;
  int want[4], cat;
  __device__ __forceinline__ explicit ScopeCate(const ScopeArgs& s) : row_cate(s.row_cate), cat(-1) {}
  __device__ __forceinline__ void row(int i, int u, int B) { want[i] = (row_cate && u < B) ? row_cate[u] : -1; }
  __device__ __forceinline__ void col(const EvalArgs& a, int item) { cat = row_cate ? a.p.item_cate[item] : -1; }
  __device__ __forceinline__ bool may(int i) const { return want[i] < 0 || cat == want[i]; }
};

// The model's score for topk_scan: fl(fl(acc * P) + bias), k_eval_topk's two roundings (eval_score).
struct ScopedScore {
  const EvalArgs& a;
  const float P;
  ScopeCate sc;
  float bias;
  f32x4 acc;
  __device__ __forceinline__ explicit ScopedScore(const ScopedTopkArgs& s) : a(s.t.e), P(eval_scale(s.t.e)), sc(s.s) {}
  __device__ __forceinline__ bool row(int i, int u) {
    sc.row(i, u, a.B);
    return u < a.B;
  }
  __device__ __forceinline__ void col(const f32x4& tile, int item) {
    acc = tile;
    bias = a.p.item_b[(size_t)item * a.p.ld_itemb];
    sc.col(a, item);
  }
  __device__ __forceinline__ float score(int i) const { return eval_score(acc[i], P, bias); }
  __device__ __forceinline__ bool may(int i, int) const { return sc.may(i); }
};

// SimScore with the category test.
struct ScopedSim {
  SimScore s;
  ScopeCate sc;
  __device__ __forceinline__ explicit ScopedSim(const ScopedSimArgs& a) : s(a.m), sc(a.s) {}
  __device__ __forceinline__ bool row(int i, int u) {
    sc.row(i, u, s.sa.t.e.B);
    return s.row(i, u);
  }
  __device__ __forceinline__ void col(const f32x4& tile, int item) {
    s.col(tile, item);
    sc.col(s.sa.t.e, item);
  }
  __device__ __forceinline__ float score(int i) const { return s.score(i); }
  __device__ __forceinline__ bool may(int i, int gn) const { return s.may(i, gn) && sc.may(i); }
};

// grid (ceil(B/16), slices of the scope's count)
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_scoped_topk(ScopedTopkArgs sa) {
  __shared__ TopkSmem<KP, BUF> sm;
  ScopedScore pol(sa);
  const ScopeMap map(sa.s, sa.t.e);
  topk_scan<D, KP, BUF, false>(sm, sa.t, pol, map);
}

template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_scoped_similar(ScopedSimArgs sa) {
  __shared__ TopkSmem<KP, BUF> sm;
  ScopedSim pol(sa);
  const ScopeMap map(sa.s, sa.m.t.e);
  topk_scan<D, KP, BUF, false>(sm, sa.m.t, pol, map);
}

// The inv pass of a scoped cosine list: k_sim_prep's lanes and sim_inv_norm for the scope's items only, 16 lanes per
// position, written at inv[local] (SimScore reads it by local item).  An index outside the table writes nothing.
template <int D>
__global__ __launch_bounds__(256) void k_scope_inv(EvalArgs a, ScopeArgs s, float* inv) {
  const ScopeMap map(s, a);
  const int cnt = map.count(a);
  const int n = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const int loc = map.local(min(n, cnt - 1));      // (whole rows stay in the butterfly)
  const int item = map.holds(loc) ? loc : 0;
  f32x4 v[D / 64];
#pragma unroll
  for (int j = 0; j < D / 64; ++j) v[j] = all_emb4(a, item, 64 * j + 4 * c);
  const float w = sim_inv_norm<D>(v);
  if (n < cnt && map.holds(loc) && c == 0) inv[item] = w;
}

// tlsan_lists.h -- indexed lists: the K best items of the UNION of a few item lists per row, where the lists are a
// caller's index of the table's items (a partition by category: model.py's CategoryIndex; any partition serves) and
// row b names up to LISTS_PMAX of them in row_lists[b, :].  Only the probed lists are scored: a row costs what its
// lists' items cost, not what the table costs (tlsan_scope.h's category test narrows what is selected, not what is
// scanned).
//
// A (row, probe) PAIR t = b * P + p is valid when 0 <= row_lists[t] < nlists, no earlier probe of the row names the
// same list (a repeat counts once, so a row's lists stay disjoint for the merge) and the list is not empty.  The call
// groups the valid pairs by list, on the device, into GROUPS of up to 16 pairs that share a list (the three kernels are
// tlsan_lists.hip's, behind tlsan_launch_lists_group):
//   k_lists_count   rank[t] = the pair's arrival number among its list's pairs (an atomic counter per list), or -1
//   k_lists_groups  gbase[c] = exclusive sum of ceil(cnt[c] / 16) over the lists (one workgroup), *ngroups = the total
//   k_lists_place   pair t sits in group gbase[c] + rank / 16 at slot rank % 16; slot 0 names the group's list
// Which pairs share a group, and in which slots, follows the arrival order and differs from call to call; no result
// depends on it, because a slot's selection state (its kept list, buffer and threshold) is its own: a pair's list is a
// function of (its row, its list, the slice) alone.  The group count is at most N / 16 + min(nlists, N), N = B * P: the
// host sizes the grid by that bound, and a workgroup past *ngroups leaves at once.
//
// The scan is topk_scan's (tlsan_topk.h) with three changes, in a text of its own so that topk_scan and the kernels on it
// keep their code: the rows of a workgroup are its group's pairs' rows (user fragment, exclusion offsets, policy rows and
// the output slot all come from pair / P, never from 16 * blockIdx.x); the item mapping has a per-workgroup base and
// count (positions list_off[c] .. list_off[c + 1] of list_items, through ScopeMap's holds: an entry outside [0, I) is
// never read as a table row and never selected); and a pair's slice list goes to [N, slices, K] at pair t, which is
// [B, P * slices, K]: k_topk_merge folds a row's P * slices lists.  Every slot of that array is filled with -1 / -inf
// before the scan, so a pair that was never scheduled, and a slice that starts past its list's end (its workgroup
// leaves at once), hold an empty list.  The slice count comes from the host's max_list: no device value sizes a grid.
// Scores: ListScore is ScopedScore and SimScore is ScopedSim without the category test (membership of the list
// replaces it), on score_tiles4's gather form: the bits of tlsan_eval_topk_scoped / tlsan_similar_topk_scoped.
// (tlsan_shelves.h holds one more copy of this loop, inside a loop over lists: a fix to either goes into both.)
#pragma once
#include "tlsan_similar.h"

#define LISTS_PMAX 8

struct ListsArgs {
  const int32_t* list_off;    // [nlists + 1]
  const int32_t* list_items;  // local item indices, list c at list_off[c] .. list_off[c + 1]
  const int32_t* row_lists;   // [N] = [B, P]
  int32_t nlists, P, N;
  int32_t* cnt;               // [nlists] valid pairs per list (zeroed before k_lists_count)
  int32_t* gbase;             // [nlists] first group of a list
  int32_t* ngroups;           // [1]
  int32_t* rank;              // [N]
  int32_t* glist;             // [groups] the list of a group
  int32_t* gpair;             // [groups, 16] the pairs of a group (slots past its count: not written)
};

struct ListsTopkArgs { TopkArgs t; ListsArgs l; };
struct ListsSimArgs { SimArgs m; ListsArgs l; };

// topk_scan's item mapping of one list (ScopeMap with a base and a count of the workgroup's own)
struct ListMap {
  const int32_t* items;
  const int n, I;
  __device__ __forceinline__ ListMap(const int32_t* items_, int n_, int I_) : items(items_), n(n_), I(I_) {}
  __device__ __forceinline__ int local(int pos) const { return items[pos]; }
  __device__ __forceinline__ bool holds(int loc) const { return (unsigned)loc < (unsigned)I; }
};

// ScopedScore without the category test
struct ListScore {
  const EvalArgs& a;
  const float P;
  float bias;
  f32x4 acc;
  __device__ __forceinline__ explicit ListScore(const ListsTopkArgs& s) : a(s.t.e), P(eval_scale(s.t.e)) {}
  __device__ __forceinline__ explicit ListScore(const EvalArgs& e) : a(e), P(eval_scale(e)) {}   // (tlsan_shelves.h)
  __device__ __forceinline__ bool row(int, int u) { return u < a.B; }
  __device__ __forceinline__ void col(const f32x4& tile, int item) {
    acc = tile;
    bias = a.p.item_b[(size_t)item * a.p.ld_itemb];
  }
  __device__ __forceinline__ float score(int i) const { return eval_score(acc[i], P, bias); }
  __device__ __forceinline__ bool may(int, int) const { return true; }
};

// The pair of slot j of group g (np pairs), -1 past them; its row, or B (no row: every policy refuses it).
__device__ __forceinline__ int lists_pair(const ListsArgs& l, int g, int np, int j) { return j < np ? l.gpair[(size_t)g * 16 + j] : -1; }
__device__ __forceinline__ int lists_row(const ListsArgs& l, int pair, int B) { return pair < 0 ? B : pair / l.P; }

// topk_finish with the output slot of each kept list taken from its pair: out[(pair * nl + y) * K + j]
template <int KP, int BUF>
__device__ __forceinline__ void lists_finish(TopkSmem<KP, BUF>& sm, const ListsArgs& l, int g, int np, int K, int nl, int y,
                                             int32_t* ids, float* scores) {
  bool left = false;
#pragma unroll
  for (int u = 0; u < 16; ++u) left |= sm.cnt[u] != 0;
  if (left) topk_reselect(sm);
  for (int p = threadIdx.x; p < 16 * K; p += 256) {
    const int u = p / K, j = p % K;
    const int pair = lists_pair(l, g, np, u);
    if (pair < 0) continue;
    const topk_key_t key = sm.kept[u][j];
    const size_t o = ((size_t)pair * nl + y) * K + j;
    ids[o] = topk_key_id(key);
    scores[o] = topk_key_score(key);
  }
}

// A workgroup of grid (groups bound, slices): group g = blockIdx.x walks its list's positions of slice y = blockIdx.y,
// n0 = (round * slices + y) * 256 + 64 w for wavefront w (topk_scan's tiling and loop, its loaded-mapping branch).
template <int D, int KP, int BUF, class Policy>
__device__ __forceinline__ void lists_scan(TopkSmem<KP, BUF>& sm, const TopkArgs& ta, const ListsArgs& l, Policy& pol) {
  const EvalArgs& a = ta.e;
  const int g = blockIdx.x;
  if (g >= l.ngroups[0]) return;                       // (past the real group count; uniform)
  const int c = l.glist[g];
  const int base = l.list_off[c];
  const int cnt = l.list_off[c + 1] - base;
  const int step = gridDim.y * 256;
  if ((int)blockIdx.y * 256 >= cnt) return;            // (the slice starts past the list's end: its lists stay as filled)
  const int np = min(16, l.cnt[c] - 16 * (g - l.gbase[c]));
  const ListMap map(l.list_items + base, cnt, a.I);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  topk_init(sm);
  f32x4 af[D / 16];
  load_user_frag<D>(a, lists_row(l, lists_pair(l, g, np, r), a.B), q, 0, af);
  bool uv[4];
  int xlo[4], xhi[4];
  topk_key_t thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = lists_row(l, lists_pair(l, g, np, 4 * q + i), a.B);
    uv[i] = pol.row(i, u);
    xlo[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u] : 0;
    xhi[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u + 1] : 0;
    thr[i] = 0ull;
  }
  __syncthreads();
  const int nround = (cnt + step - 1) / step;
  const int w0 = (blockIdx.y * 4 + wave) * 64;
  auto locals = [&](int n0, int (&loc)[4]) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) loc[tt] = map.local(min(n0 + 16 * tt + r, cnt - 1));
  };
  int nxt[4] = {0, 0, 0, 0};   // the coming round's
  if (w0 < cnt) locals(w0, nxt);
  int ph = 0;
  for (int rd = 0; rd < nround; ++rd) {
    const int n0 = rd * step + w0;
    topk_key_t key[16];
    unsigned pend = 0;
    if (n0 < cnt) {
      int item[4];
      bool held[4];
      f32x4 acc[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        held[tt] = map.holds(nxt[tt]);
        item[tt] = held[tt] ? nxt[tt] : 0;
      }
      if (n0 < cnt - step) locals(n0 + step, nxt);
      score_tiles4<D, false>(a, af, item, q, acc);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const bool vn = n0 + 16 * tt + r < cnt && held[tt];
        const int gn = item[tt] * a.id_mul + a.id_add;  // global item id
        pol.col(acc[tt], item[tt]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          key[4 * tt + i] = topk_key(pol.score(i), gn);
          // (the exclusion list is searched only for scores that pass the threshold)
          if (vn && uv[i] && pol.may(i, gn) && key[4 * tt + i] > thr[i] && !topk_in_list(ta.excl_ids, xlo[i], xhi[i], gn))
            pend |= 1u << (4 * tt + i);
        }
      }
    }
    topk_offer(sm, key, pend, 4 * q, thr, ta.K, ph);
  }
  lists_finish(sm, l, g, np, ta.K, gridDim.y, blockIdx.y, ta.ids, ta.scores);
}

template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_lists_topk(ListsTopkArgs la) {
  __shared__ TopkSmem<KP, BUF> sm;
  ListScore pol(la);
  lists_scan<D, KP, BUF>(sm, la.t, la.l, pol);
}

template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_lists_similar(ListsSimArgs la) {
  __shared__ TopkSmem<KP, BUF> sm;
  SimScore pol(la.m);
  lists_scan<D, KP, BUF>(sm, la.m.t, la.l, pol);
}

// The inv pass of an indexed cosine list: k_scope_inv's lanes and sim_inv_norm over every position of the index
// (list_off[nlists] of them, read here: the grid is sized by the table and strides), written at inv[local].  An entry
// outside the table writes nothing; an item two lists hold is written twice with the same value.
template <int D>
__global__ __launch_bounds__(256) void k_lists_inv(EvalArgs a, ListsArgs l, float* inv) {
  const int total = l.list_off[l.nlists];
  const int c = threadIdx.x & 15;
  for (int n0 = blockIdx.x * 16; n0 < total; n0 += gridDim.x * 16) {   // (uniform: whole rows stay in the butterfly)
    const int n = n0 + (threadIdx.x >> 4);
    const int loc = l.list_items[min(n, total - 1)];
    const bool held = (unsigned)loc < (unsigned)a.I;
    const int item = held ? loc : 0;
    f32x4 v[D / 64];
#pragma unroll
    for (int j = 0; j < D / 64; ++j) v[j] = all_emb4(a, item, 64 * j + 4 * c);
    const float w = sim_inv_norm<D>(v);
    if (n < total && held && c == 0) inv[item] = w;
  }
}

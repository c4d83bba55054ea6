// tlsan_listm.h -- list metrics: what a recommendation list looks like beside its accuracy.  A row is a list of K <= 256
// entries (global id g_j, -1 = no entry, anywhere; stored vector w_j, inv_j of sim_inv_norm, category c_j -- the staging
// of tlsan_rerank) and gives, over its valid entries (g_j >= 0) in position order:
//
//   n_valid     their number n
//   cos(i, j)   fl(dot(i, j) * fl(inv_i * inv_j)), tlsan_rerank's: lane c of a DPP row chains the FMAs of columns
//               64 q + 4 c .. + 3, q ascending, the 16 partials meet in lanes_sum<16>
//   pair_cos    sum over valid i < j of cos(i, j) in double, in ONE order: entry j owns c_j = ((0 + cos(i0, j)) + cos(i1, j))
//               + ..., its valid i < j ascending; pair_cos = ((0 + c_0) + c_1) + ... + c_{K-1}, j ascending, an entry
//               that is not valid holding c_j = 0.  The order names no thread: it is the same for both block sizes
//   n_cate      distinct categories; max_cate: the most entries sharing one (0 for an empty row)
//   hit_pos     first position j (holes counted) with g_j == labels[b] >= 0, else -1
//   weight_sum  ((0 + weight[j0]) + weight[j1]) + ... in double over the valid j ascending; 0 without weights
//   exposure    exposure[g_j] += 1 (integer atomic) for the valid entries with g_j < n_items
//
// One workgroup per row in k_rerank's layout: 16 lanes of a DPP row per vector in f32x4 pieces, four entries per 16-lane
// group held in registers (entry j: group j % G, slot j / G, G = threads / 16).  The K broadcast rounds have no
// dependent step between them, so LISTM_T entries' vectors go through LDS per barrier, double-buffered (the round that
// computes against buffer s & 1 has buffer (s + 1) & 1 written behind the same barrier): a step is  barrier [owners of
// entries (s + 1) T .. write theirs] [every group: its slots' dots against entries s T .. + T - 1, added to c_j where
// i < j and both are valid].  A slot whose entries all lie at or below i, and an i that is not valid, are skipped by the
// whole workgroup.  The category statistics are integer compares of one thread per entry over the [K] list in LDS; the
// integers meet in LDS integer atomics (order-free).  No floating-point atomics, no K x K matrix: a row's bits depend on
// its list alone.  256 threads serve K <= 64, 1024 threads K <= 256.
#pragma once
#include "tlsan_eval.h"

#define LISTM_MAX 256   // largest list (TOPK_MAX / RERANK_MAX: what recommend can deliver)
#define LISTM_EPG 4     // entries per 16-lane group
#define LISTM_T 8       // entries whose vectors pass through LDS per barrier

struct ListmArgs {
  const int32_t* ids;          // [B, K]
  const float* vec;            // [B * K, D]
  const float* inv;            // [B * K]
  const int32_t* cate;         // [B * K]
  const int32_t* labels;       // [B] or NULL
  const float* weight;         // [B * K] or NULL
  int32_t B, K, n_items;
  int32_t* n_valid;            // [B]
  double* pair_cos;            // [B]
  int32_t* n_cate;             // [B]
  int32_t* max_cate;           // [B]
  int32_t* hit_pos;            // [B]
  double* weight_sum;          // [B]
  uint32_t* exposure;          // [n_items] or NULL
};

template <int D>
struct ListmSmem {
  alignas(16) float sel[2][LISTM_T][D];   // the vectors of a step's entries, two steps
  double c[LISTM_MAX];                    // c_j
  float inv[LISTM_MAX];                   // 0 for an entry that is not valid
  float wt[LISTM_MAX];                    // the entry's weight, 0 for an entry that is not valid (x + 0 == x: skipped or added, the same bits)
  int32_t id[LISTM_MAX];
  int32_t cate[LISTM_MAX];
  int32_t n_valid, n_cate, max_cate, hit_pos;
};

// grid B, block NT (256: K <= 64; 1024: K <= 256)
template <int D, int NT>
__global__ __launch_bounds__(NT) void k_list_metrics(ListmArgs a) {
#pragma clang fp contract(off)
  constexpr int G = NT / 16, E = LISTM_EPG, Q = D / 64, T = LISTM_T;
  static_assert(G % T == 0, "a step's entries share one slot");   // (the launcher keeps K <= G * E)
  __shared__ ListmSmem<D> sm;
  const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15;
  const int K = a.K;
  const size_t row = blockIdx.x;

  // (every load below is issued whatever the ids hold -- an address never waits for a loaded id -- and masked afterwards)
  const int32_t lab = a.labels != nullptr ? a.labels[row] : -1;
  for (int j = tid; j < LISTM_MAX; j += NT) {
    const bool in = j < K;
    const size_t p = row * K + (in ? j : 0);
    const int32_t g = a.ids[p], ct = a.cate[p];
    const float iv = a.inv[p], wv = a.weight != nullptr ? a.weight[p] : 0.0f;
    const bool v = in && g >= 0;
    sm.id[j] = v ? g : -1;
    sm.inv[j] = v ? iv : 0.0f;
    sm.cate[j] = v ? ct : 0;
    sm.wt[j] = v ? wv : 0.0f;
  }
  if (tid == 0) { sm.n_valid = 0; sm.n_cate = 0; sm.max_cate = 0; sm.hit_pos = LISTM_MAX; }
  // this group's entries: vector pieces, inv, validity
  f32x4 w[E][Q];
  float inv[E];
  bool ok[E];
  double cj[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = e * G + grp;
    const bool in = j < K;
    const size_t p = row * K + (in ? j : 0);
    const float iv = a.inv[p];
    ok[e] = in && a.ids[p] >= 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      w[e][q] = *(const f32x4*)(a.vec + p * D + 64 * q + 4 * c);
      if (!ok[e]) w[e][q] = (f32x4)(0.0f);
    }
    inv[e] = ok[e] ? iv : 0.0f;
    cj[e] = 0.0;
  }
  // the vectors of entries s T .. s T + T - 1 (one slot, T consecutive groups) -> buffer s & 1
  auto publish = [&](int s) {
    const int i0 = s * T, es = i0 / G, t = grp - i0 % G;
    if (t >= 0 && t < T) {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (e == es) {
#pragma unroll
          for (int q = 0; q < Q; ++q) *(f32x4*)(&sm.sel[s & 1][t][64 * q + 4 * c]) = w[e][q];
        }
    }
  };
  const int nsteps = (K - 1 + T - 1) / T;     // entry K - 1 has no j behind it
  if (nsteps > 0) publish(0);
  __syncthreads();

  // ---- the integers and the weights: one thread per entry
  if (tid < K) {
    const int32_t g = sm.id[tid];
    if (g >= 0) {
      const int32_t mine = sm.cate[tid];
      int same = 0, before = 0;
      for (int i = 0; i < K; ++i) {
        const bool m = sm.id[i] >= 0 && sm.cate[i] == mine;
        same += m;
        before += m && i < tid;
      }
      atomicAdd(&sm.n_valid, 1);
      if (before == 0) atomicAdd(&sm.n_cate, 1);
      atomicMax(&sm.max_cate, same);
      if (lab >= 0 && g == lab) atomicMin(&sm.hit_pos, tid);
      if (a.exposure != nullptr && g < a.n_items) atomicAdd(a.exposure + g, 1u);
    }
  }
  if (tid == NT - 64) {                        // (a wavefront the integers above keep least busy)
    double ws = 0.0;
    for (int j = 0; j < K; ++j) ws += (double)sm.wt[j];
    a.weight_sum[row] = ws;
  }

  // ---- the pairs
  for (int s = 0; s < nsteps; ++s) {
    if (s > 0) __syncthreads();
    if (s + 1 < nsteps) publish(s + 1);
#pragma unroll 2
    for (int t = 0; t < T; ++t) {
      const int i = s * T + t;
      if (i >= K - 1) break;
      if (sm.id[i] < 0) continue;              // (the same for the whole workgroup)
      const float inv_i = sm.inv[i];
      f32x4 x[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) x[q] = *(const f32x4*)(&sm.sel[s & 1][t][64 * q + 4 * c]);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (e * G + G - 1 > i) {               // (the slot still holds an entry behind i)
          float p = 0.0f;
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) p = __builtin_fmaf(w[e][q][k], x[q][k], p);
          const float cs = lanes_sum<16>(p) * (inv_i * inv[e]);
          if (ok[e] && e * G + grp > i) cj[e] += (double)cs;
        }
      }
    }
  }
  if (c == 0) {
#pragma unroll
    for (int e = 0; e < E; ++e) sm.c[e * G + grp] = cj[e];   // (G * E <= LISTM_MAX)
  }
  __syncthreads();
  if (tid == 0) {
    double pc = 0.0;
    for (int j = 0; j < K; ++j) pc += sm.c[j];
    a.pair_cos[row] = pc;
    a.n_valid[row] = sm.n_valid;
    a.n_cate[row] = sm.n_cate;
    a.max_cate[row] = sm.max_cate;
    a.hit_pos[row] = sm.hit_pos < LISTM_MAX ? sm.hit_pos : -1;
  }
}

hipError_t tlsan_launch_list_metrics(const ListmArgs& a, int D, hipStream_t hs);

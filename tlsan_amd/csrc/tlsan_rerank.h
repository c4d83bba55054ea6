// tlsan_rerank.h -- diversified lists: the second stage behind tlsan_eval_topk.  From a row's pool of N <= 256 entries
// (global id g_j, model score s_j, stored vector w_j, inv_j of sim_inv_norm, category c_j; tlsan_eval_topk's order) pick
// K by greedy maximal marginal relevance under a per-category cap:
//
//   valid      g_j >= 0 and s_j finite; the others are never selected
//   r_j        (s_j - s_lo) / (s_hi - s_lo), s_hi / s_lo the scores of the first / last valid entry; 0 when they are equal
//   cos(i, j)  fl(dot(i, j) * fl(inv_i * inv_j)), dot the fp32 sum of w_i[k] w_j[k] in the order of sim_inv_norm: lane c of
//              a DPP row chains the FMAs of columns 64 q + 4 c .. + 3, q ascending, the 16 partials meet in lanes_sum<16>
//   step t     eligible: valid, not selected, and (m > 0) fewer than m selected entries of its category;
//              v_j = fl((1 - theta) r_j) for the first pick, then fl(fl((1 - theta) r_j) - fl(theta * max_i cos(i, j)))
//              over the selected i; the eligible entry of largest v_j is picked, equal values (+0 == -0) -> lower position;
//              nobody eligible: the row ends, the rest is id -1 / score -inf
//   theta = 0  v_j = r_j: no product is formed, the selection is integer logic on the scores' order
//
// One workgroup per row, 16 lanes of a DPP row per vector and four entries per 16-lane group (entry j: group j % G,
// slot j / G, G = threads / 16): every vector stays in registers for the whole loop (d / 4 <= 64 per lane).  A step is
// K dependent rounds of  [each group's best key -> LDS] barrier [every wavefront reduces the G keys: same winner
// everywhere; its group writes the vector, inv and category to LDS and the output] barrier [every group: four dots
// against the winner, its max cosine and its category count].  No atomics, no N x N matrix; every order is fixed by
// (d, lane), so a row's bits depend on its pool alone.  256 threads serve N <= 64, 1024 threads N <= 256; both give the
// same bits (the dot's order and the exact argmax do not depend on G).
#pragma once
#include "tlsan_eval.h"

#define RERANK_MAX 256   // largest pool (TOPK_MAX: what tlsan_eval_topk can deliver)
#define RERANK_EPG 4     // entries per 16-lane group

struct RerankArgs {
  const int32_t* pool_ids;     // [B, N]
  const float* pool_scores;    // [B, N]
  const float* vec;            // [B * N, D]
  const float* inv;            // [B * N]
  const int32_t* cate;         // [B * N]
  int32_t B, N, K, per_category;
  float diversity;
  int32_t* ids;                // [B, K]
  float* scores;               // [B, K]
};

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

// max of a 64-bit key (hi, lo) over the wavefront, the same in every lane: the butterfly of lanes_sum<16> inside each
// row (max is exact and idempotent: any tree gives the same key), then the four rows' keys by v_readlane
__device__ __forceinline__ void wave_max_key(uint32_t& hi, uint32_t& lo) {
#define RERANK_STEP(CTRL)                                           \
  do {                                                              \
    const uint32_t oh = dpp_u32<CTRL>(hi), ol = dpp_u32<CTRL>(lo);  \
    const bool take = oh > hi || (oh == hi && ol > lo);             \
    hi = take ? oh : hi;                                            \
    lo = take ? ol : lo;                                            \
  } while (0)
  RERANK_STEP(TLSAN_DPP_XOR1);
  RERANK_STEP(TLSAN_DPP_XOR2);
  RERANK_STEP(TLSAN_DPP_HMIRROR);
  RERANK_STEP(TLSAN_DPP_MIRROR);
#undef RERANK_STEP
  uint32_t bh = __builtin_amdgcn_readlane(hi, 0), bl = __builtin_amdgcn_readlane(lo, 0);
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    const uint32_t oh = __builtin_amdgcn_readlane(hi, 16 * r), ol = __builtin_amdgcn_readlane(lo, 16 * r);
    const bool take = oh > bh || (oh == bh && ol > bl);
    bh = take ? oh : bh;
    bl = take ? ol : bl;
  }
  hi = bh;
  lo = bl;
}

// a float as an unsigned key of the same order, -inf and up >= 1 (0 is left for "not eligible"); -0 counts as +0 and a
// NaN as -inf
__device__ __forceinline__ uint32_t rerank_key(float v) {
  v = v == v ? v + 0.0f : -INFINITY;
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct RerankSmem {
  float score[RERANK_MAX];     // the pool's scores (prologue: s_hi, s_lo)
  int32_t id[RERANK_MAX];
  uint32_t key_hi[64], key_lo[64];   // a group's best of the step
  alignas(16) float sel[256];  // the winner's vector
  float sel_inv;
  int32_t sel_cate;
};

// grid B, block NT (256: N <= 64; 1024: N <= 256)
template <int D, int NT>
__global__ __launch_bounds__(NT) void k_rerank(RerankArgs a) {
#pragma clang fp contract(off)
  constexpr int G = NT / 16, E = RERANK_EPG, Q = D / 64;
  __shared__ RerankSmem sm;
  const int tid = threadIdx.x, grp = tid >> 4, c = tid & 15, lane = tid & 63;
  const int N = a.N, K = a.K, m = a.per_category;
  const size_t row = blockIdx.x;
  const float theta = a.diversity;

  for (int j = tid; j < RERANK_MAX; j += NT) {
    sm.score[j] = j < N ? a.pool_scores[row * N + j] : -INFINITY;
    sm.id[j] = j < N ? a.pool_ids[row * N + j] : -1;
  }
  // this group's entries: vector pieces, inv, category, score, id
  f32x4 w[E][Q];
  float inv[E], s[E];
  int32_t cat[E], gid[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = e * G + grp;
    const bool in = j < N;
    const size_t p = row * N + (in ? j : 0);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      w[e][q] = *(const f32x4*)(a.vec + p * D + 64 * q + 4 * c);
      if (!in) w[e][q] = (f32x4)(0.0f);
    }
    inv[e] = in ? a.inv[p] : 0.0f;
    cat[e] = in ? a.cate[p] : -1;
    s[e] = in ? a.pool_scores[p] : -INFINITY;
    gid[e] = in ? a.pool_ids[p] : -1;
  }
  __syncthreads();
  // first and last valid entry, by every wavefront for itself
  uint32_t fk = 0, lk = 0;
#pragma unroll
  for (int i = 0; i < RERANK_MAX / 64; ++i) {
    const int j = 64 * i + lane;
    const float sj = sm.score[j];
    if (sm.id[j] >= 0 && fabsf(sj) < INFINITY) {   // (false for a NaN)
      fk = max(fk, (uint32_t)(RERANK_MAX - j));
      lk = max(lk, (uint32_t)(j + 1));
    }
  }
  uint32_t zero = 0;
  wave_max_key(fk, zero);
  zero = 0;
  wave_max_key(lk, zero);
  int t = 0;
  if (fk != 0) {
    const float s_hi = sm.score[RERANK_MAX - (int)fk], s_lo = sm.score[(int)lk - 1];
    const float span = s_hi - s_lo, keep = 1.0f - theta;
    float rel[E], mc[E];        // fl((1 - theta) r_j); max cosine against the selected
    int32_t cnt[E];             // selected entries of this entry's category
    bool open[E];               // valid and not selected
#pragma unroll
    for (int e = 0; e < E; ++e) {
      open[e] = gid[e] >= 0 && fabsf(s[e]) < INFINITY;
      rel[e] = keep * (span == 0.0f ? 0.0f : (s[e] - s_lo) / span);
      mc[e] = -INFINITY;
      cnt[e] = 0;
    }
    for (; t < K; ++t) {
      uint32_t bh = 0, bl = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (open[e] && (m == 0 || cnt[e] < m)) {
          const float v = (t == 0 || theta == 0.0f) ? rel[e] : rel[e] - theta * mc[e];
          const uint32_t kh = rerank_key(v), kl = 0xFFFFFFFFu - (uint32_t)(e * G + grp);
          if (kh > bh || (kh == bh && kl > bl)) { bh = kh; bl = kl; }
        }
      }
      if (c == 0) { sm.key_hi[grp] = bh; sm.key_lo[grp] = bl; }
      __syncthreads();
      bh = lane < G ? sm.key_hi[lane] : 0;
      bl = lane < G ? sm.key_lo[lane] : 0;
      wave_max_key(bh, bl);
      if (bh == 0) break;                       // (the same keys in every wavefront: the workgroup leaves together)
      const int win = (int)(0xFFFFFFFFu - bl), we = win / G;
      if (grp == win % G) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (e == we) {
#pragma unroll
            for (int q = 0; q < Q; ++q) *(f32x4*)(sm.sel + 64 * q + 4 * c) = w[e][q];
            if (c == 0) {
              sm.sel_inv = inv[e];
              sm.sel_cate = cat[e];
              a.ids[row * K + t] = gid[e];
              a.scores[row * K + t] = s[e];
            }
            open[e] = false;
          }
        }
      }
      __syncthreads();
      if (t + 1 == K) { ++t; break; }
      const int wc = sm.sel_cate;
#pragma unroll
      for (int e = 0; e < E; ++e) cnt[e] += cat[e] == wc;
      if (theta != 0.0f) {
        const float winv = sm.sel_inv;
        f32x4 x[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = *(const f32x4*)(sm.sel + 64 * q + 4 * c);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          float p = 0.0f;
#pragma unroll
          for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) p = __builtin_fmaf(w[e][q][i], x[q][i], p);
          mc[e] = fmaxf(mc[e], lanes_sum<16>(p) * (winv * inv[e]));
        }
      }
    }
  }
  for (int i = t + tid; i < K; i += NT) {       // a row that ran out of eligible entries
    a.ids[row * K + i] = -1;
    a.scores[row * K + i] = -INFINITY;
  }
}

hipError_t tlsan_launch_rerank(const RerankArgs& a, int D, hipStream_t hs);

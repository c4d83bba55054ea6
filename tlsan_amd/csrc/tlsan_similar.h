// tlsan_similar.h -- similar-items lists: for each query item the K nearest items of the table by dot product or cosine
// of the representation the model scores with, w_n = [item_emb[n] || cate_emb[item_cate[n]]] (the matrix k_all_emb
// builds), selected inside the scoring kernel by k_eval_topk's loop in its shared form (topk_scan): the [Q, I] similarity matrix is never materialised.
//
//   acc(q, n)  the fp32 MFMA accumulation of w_q . w_n on STORED values: the chains of k_eval_topk's tiles, the
//              query's stored vector in the place of u_t.  The products commute and the k-order is the chain's, so
//              acc(a, b) and acc(b, a) are the same float.
//   inv(n)     1 / sqrtf(ss_n), ss_n = sum_k w_n[k]^2 in fp32 in the one order of sim_inv_norm; 0 when ss_n == 0
//   dot        s = fl(acc * fl(P * P))                (P the table scale: the product of the true vectors)
//   cosine     s = fl(acc * fl(inv(q) * inv(n)))      (P cancels)
// No bias.  Order and keys are tlsan_topk.h's; the query's own id and the row's exclusion list are never selected.
#pragma once
#include "tlsan_topk.h"

#define SIM_DOT 0      // TLSAN_SIM_DOT / TLSAN_SIM_COSINE (include/tlsan.h)
#define SIM_COSINE 1

struct SimArgs {
  TopkArgs t;              // e.u_t = the queries' stored vectors [Q, D], e.B = Q; K, exclusion lists, outputs as top-K's
  const float* qinv;       // [Q] inv of the queries (cosine; NULL for dot)
  const int32_t* qids;     // [Q] global ids of the queries; < 0 (whole table: or >= I): a padding row
  const float* inv;        // [I] inv of the table's items (cosine; the inv pass of this call)
  int32_t metric;
};

struct VecArgs {           // k_item_vectors
  EvalArgs e;              // p, I, di, dc, id_mul, id_add
  const int32_t* ids;      // [Q] global ids
  int32_t Q;
  float* vec;              // [Q, D]
  float* inv;              // [Q] or NULL
};

// Sum of squares of item `it`'s stored vector and its inverse norm, by the 16 lanes of a DPP row: lane c holds columns
// 64 j + 4 c .. + 3 (pieces v[j], j < D / 64), squares them in column order into one fp32 partial with explicit FMAs, and
// the partials meet in lanes_sum<16>'s butterfly.  THE one definition of inv for queries and table items alike: the
// order is fixed by (D, lane), not by the launch, and every operation is correctly rounded (no contraction left to the
// compiler), so the same stored row gives the same bits wherever it is computed.  Every lane of the row gets the value.
template <int D>
__device__ __forceinline__ float sim_inv_norm(const f32x4 (&v)[D / 64]) {
#pragma clang fp contract(off)
  float p = 0.0f;
#pragma unroll
  for (int j = 0; j < D / 64; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) p = __builtin_fmaf(v[j][s], v[j][s], p);
  const float ss = lanes_sum<16>(p);
  return ss == 0.0f ? 0.0f : 1.0f / sqrtf(ss);
}

// The inv pass: 16 lanes per table item, 16 items per workgroup; also writes the dense [I, D] matrix when there is one
// (k_all_emb's values: one read of the tables for both).
template <int D>
__global__ __launch_bounds__(256) void k_sim_prep(EvalArgs a, float* inv) {
  const int it = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const int item = min(it, a.I - 1);      // (whole rows stay in the butterfly)
  f32x4 v[D / 64];
#pragma unroll
  for (int j = 0; j < D / 64; ++j) v[j] = all_emb4(a, item, 64 * j + 4 * c);
  const float w = sim_inv_norm<D>(v);
  if (it >= a.I) return;
  if (a.all_emb) {
#pragma unroll
    for (int j = 0; j < D / 64; ++j) *(f32x4*)(a.all_emb + (size_t)it * D + 64 * j + 4 * c) = v[j];
  }
  if (c == 0) inv[it] = w;
}

// tlsan_item_vectors: the stored vector and inv of query ids[q] when this table holds it (global id n * id_mul + id_add),
// zeros otherwise.  Same lanes, same sim_inv_norm.
template <int D>
__global__ __launch_bounds__(256) void k_item_vectors(VecArgs va) {
  const EvalArgs& a = va.e;
  const int qi = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const int g = qi < va.Q ? va.ids[qi] : -1;
  const int rel = g - a.id_add;
  const bool held = g >= 0 && rel >= 0 && rel % a.id_mul == 0 && rel / a.id_mul < a.I;
  const int item = held ? rel / a.id_mul : 0;
  f32x4 v[D / 64];
#pragma unroll
  for (int j = 0; j < D / 64; ++j) {
    v[j] = all_emb4(a, item, 64 * j + 4 * c);
    if (!held) v[j] = (f32x4)(0.0f);
  }
  const float w = sim_inv_norm<D>(v);
  if (qi >= va.Q) return;
#pragma unroll
  for (int j = 0; j < D / 64; ++j) *(f32x4*)(va.vec + (size_t)qi * D + 64 * j + 4 * c) = v[j];
  if (c == 0 && va.inv) va.inv[qi] = w;
}

// The similarity score for topk_scan (tlsan_topk.h: the tiles, chains, TopkSmem and phases of k_eval_topk, which keeps
// its own text of the loop for its speed):
//   s = acc * fl(qm * nm): cosine qm = inv(q), nm = inv(n); dot qm = fl(P * P), nm = 1 (exact);
// a row is a query this table can answer (a padding row selects nothing), and no query selects its own id.
struct SimScore {
  const SimArgs& sa;
  const bool cosine, whole;
  const float P, P2;
  float qm[4], nm;
  int qid[4];
  f32x4 acc;
  __device__ __forceinline__ explicit SimScore(const SimArgs& s)
      : sa(s), cosine(s.metric == SIM_COSINE), whole(s.t.e.id_mul == 1 && s.t.e.id_add == 0), P(eval_scale(s.t.e)), P2(P * P) {}
  __device__ __forceinline__ bool row(int i, int u) {
    const EvalArgs& a = sa.t.e;
    qid[i] = u < a.B ? sa.qids[u] : -1;
    const bool v = qid[i] >= 0 && !(whole && qid[i] >= a.I);
    qm[i] = cosine ? (v ? sa.qinv[u] : 0.0f) : P2;
    return v;
  }
  __device__ __forceinline__ void col(const f32x4& tile, int item) {
    acc = tile;
    nm = cosine ? sa.inv[item] : 1.0f;
  }
  __device__ __forceinline__ float score(int i) const { return acc[i] * (qm[i] * nm); }   // (products only: nothing to fuse)
  __device__ __forceinline__ bool may(int i, int gn) const { return gn != qid[i]; }
};

// grid (ceil(Q/16), slices)
template <int D, int KP, int BUF, bool DENSE>
__global__ __launch_bounds__(256, 2) void k_similar_topk(SimArgs sa) {
  __shared__ TopkSmem<KP, BUF> sm;
  SimScore pol(sa);
  topk_scan<D, KP, BUF, DENSE>(sm, sa.t, pol, AllItems());
}

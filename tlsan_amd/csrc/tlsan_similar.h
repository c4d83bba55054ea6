// tlsan_similar.h -- similar-items lists: for each query item the K nearest items of the table by dot product or cosine
// of the representation the model scores with, w_n = [item_emb[n] || cate_emb[item_cate[n]]] (the matrix k_all_emb
// builds), selected inside the scoring kernel as k_eval_topk does: the [Q, I] similarity matrix is never materialised.
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

// grid (ceil(Q/16), slices): k_eval_topk's tile loop and selection (tlsan_topk.h: the same tiles, chains, TopkSmem and
// phases -- a copy, because k_eval_topk moved to a shared loop does not compile to the code it has now) with
//   the epilogue  s = acc * fl(qm * nm): cosine qm = inv(q), nm = inv(n); dot qm = fl(P * P), nm = 1 (exact), and
//   the eligibility test, which also rejects the query's own id and everything for a padding row.
template <int D, int KP, int BUF, bool DENSE>
__global__ __launch_bounds__(256, 2) void k_similar_topk(SimArgs sa) {
#pragma clang fp contract(off)
  __shared__ TopkSmem<KP, BUF> sm;
  const TopkArgs& ta = sa.t;
  const EvalArgs& a = ta.e;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * 16;
  topk_init(sm);
  f32x4 af[D / 16];
  load_user_frag<D>(a, u0, q, r, af);
  const bool cosine = sa.metric == SIM_COSINE;
  const float P = a.p.scale ? *a.p.scale : 1.0f;
  const float P2 = P * P;
  const bool whole = a.id_mul == 1 && a.id_add == 0;
  bool uv[4];
  int xlo[4], xhi[4], qid[4];
  float qm[4];
  topk_key_t thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = u0 + 4 * q + i;
    qid[i] = u < a.B ? sa.qids[u] : -1;
    uv[i] = qid[i] >= 0 && !(whole && qid[i] >= a.I);
    qm[i] = cosine ? (uv[i] ? sa.qinv[u] : 0.0f) : P2;
    xlo[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u] : 0;
    xhi[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u + 1] : 0;
    thr[i] = 0ull;
  }
  __syncthreads();
  const int step = gridDim.y * 256;
  const int nround = (a.I + step - 1) / step;
  int ph = 0;
  for (int rd = 0; rd < nround; ++rd) {
    const int n0 = rd * step + (blockIdx.y * 4 + wave) * 64;
    topk_key_t key[16];
    unsigned pend = 0;
    if (n0 < a.I) {
      int item[4];
      f32x4 acc[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) item[tt] = min(n0 + 16 * tt + r, a.I - 1);
      if (DENSE) {
        const float* rows[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          rows[tt] = a.all_emb + (size_t)item[tt] * D + 4 * q;
          acc[tt] = (f32x4)(0.0f);
        }
#pragma unroll
        for (int kc = 0; kc < D / 16; ++kc) {
          f32x4 bv[4];
#pragma unroll
          for (int tt = 0; tt < 4; ++tt) bv[tt] = *(const f32x4*)(rows[tt] + 16 * kc);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[tt] = TLSAN_MFMA(af[kc][s], bv[tt][s], acc[tt]);
        }
      } else {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) acc[tt] = score_tile<D>(a, af, item[tt], q);
      }
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int n = n0 + 16 * tt + r;
        const bool vn = n < a.I;
        const int gn = n * a.id_mul + a.id_add;  // global item id
        const float nm = cosine ? sa.inv[item[tt]] : 1.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = acc[tt][i] * (qm[i] * nm);
          key[4 * tt + i] = topk_key(s, gn);
          // (the exclusion list is searched only for scores that pass the threshold)
          if (vn && uv[i] && gn != qid[i] && key[4 * tt + i] > thr[i] &&
              !topk_in_list(ta.excl_ids, xlo[i], xhi[i], gn))
            pend |= 1u << (4 * tt + i);
        }
      }
    }
    for (;;) {
      bool ovf = false;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        if (!(pend & (1u << c))) continue;
        if (key[c] <= thr[c & 3] || topk_push(sm, 4 * q + (c & 3), key[c])) pend &= ~(1u << c);
        else ovf = true;
      }
      if (!topk_phase_end(sm, ovf, ph)) break;
      topk_reselect(sm);
#pragma unroll
      for (int i = 0; i < 4; ++i) thr[i] = sm.kept[4 * q + i][ta.K - 1];
    }
  }
  topk_finish(sm, u0, a.B, ta.K, gridDim.y, blockIdx.y, ta.ids, ta.scores);
}

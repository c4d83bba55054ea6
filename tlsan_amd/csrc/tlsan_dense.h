// tlsan_dense.h -- the K best rows of a dense fp32 matrix x [N, D] for each query vector q [Q, D]: topk_scan
// (tlsan_topk.h) on its dense form with the queries in u_t's place and x as the item matrix.  No table is read.  What it
// is for is the audience of an item: q the stored vectors of the query items (tlsan_item_vectors), x the users' u_t rows.
//
//   acc(q, n)    the fp32 MFMA chain of score_tiles4<D, true>: the query's vector is the A fragment, x's row the B one.
//                The products commute and the chain's k-order is the same, so this is the float a recommendation's tile
//                holds for (u_t = x[n], item vector = q) -- tlsan_similar.h makes the same remark about its own pairs.
//   score(q, n)  fl(fl(acc * scale_q) + bias_q), eval_score's two roundings (contraction is off inside eval_score): with
//                scale the table scale P and bias the query item's item_b it equals tlsan_eval_topk's and
//                tlsan_score_candidates' score of that (user row, item) pair bit for bit.
// The global id of matrix row n is id_add + n.  Order, keys, padding, NaN last and +0 == -0 are tlsan_topk.h's; a tie goes
// to the lower global row id; a row on the query's exclusion list (global row ids, ascending) is never selected, listed
// ids outside [id_add, id_add + N) match no row.  The scan is instantiated in this unit only, so the kernels of the other
// units keep their code.
#pragma once
#include "tlsan_topk.h"

struct DenseTopkArgs {
  TopkArgs t;             // e.u_t = q, e.B = Q, e.all_emb = x, e.I = N, ids id_add + n; K, exclusion lists, outputs as top-K's
  const float* q_scale;   // [Q] or NULL (1)
  const float* q_bias;    // [Q] or NULL (0)
};

// topk_scan's policy: scale and bias belong to the lane's ROW (the query), every column of the matrix may be selected.
struct DenseScore {
  const DenseTopkArgs& a;
  float sc[4], bias[4];
  f32x4 acc;
  __device__ __forceinline__ explicit DenseScore(const DenseTopkArgs& a_) : a(a_) {}
  __device__ __forceinline__ bool row(int i, int u) {
    const bool v = u < a.t.e.B;
    sc[i] = (v && a.q_scale) ? a.q_scale[u] : 1.0f;
    bias[i] = (v && a.q_bias) ? a.q_bias[u] : 0.0f;
    return v;
  }
  __device__ __forceinline__ void col(const f32x4& tile, int) { acc = tile; }
  __device__ __forceinline__ float score(int i) const { return eval_score(acc[i], sc[i], bias[i]); }
  __device__ __forceinline__ bool may(int, int) const { return true; }
};

// grid (ceil(Q / 16), slices): the slice's lists go to [Q, slices, K]
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_dense_topk(DenseTopkArgs da) {
  __shared__ TopkSmem<KP, BUF> sm;
  DenseScore pol(da);
  topk_scan<D, KP, BUF, true>(sm, da.t, pol, AllItems());
}

// tlsan_cluster.h -- a clustered item index: k-means over dense fp32 vectors (an item's [item_emb || cate_emb[item_cate]],
// as tlsan_item_vectors writes it) and the choice of the lists a query probes.  Three kernels, none of which reads a table:
//   k_cluster_assign  the nearest centroid of each row: argmax over j of x . c_j - |c_j|^2 / 2 (the Euclidean argmin without
//                     the row's own norm), on the evaluation scorers' 16 x 16 fp32 MFMA tiles -- a wavefront holds 16 rows of
//                     x as the A fragment and streams the centroids, 64 at a time, through score_tile_dense's chains
//   k_cluster_means   centroid j = the mean of the rows a segment of `order` names, summed in double in that order
//   k_cluster_probe   the P lists of highest (q . c_j) * scale_j + bias_j per row: topk_scan (tlsan_topk.h) on its dense
//                     form with the centroids as the item matrix, a policy of its own (ProbeScore) and K = P.  The scan is
//                     instantiated in this unit only, so the kernels of the other units keep their code.
// Every result is a function of the call's inputs: a row's assignment and a row's probes depend on that row and the centroids
// alone (an MFMA output row reads its own A row only; no value crosses rows), the means have one summation order and nobody
// uses a floating-point atomic.
#pragma once
#include "tlsan_topk.h"

#define CLUSTER_CMAX 16384   // most centroids of a call
#define CLUSTER_PMAX 64      // most probes of a row (the kept list of the selection: TopkSmem<64, 128>)

struct AssignArgs {
  const float* x;        // [N, D]
  const float* cent;     // [C, D]
  const float* half;     // [C] |c_j|^2 / 2 (k_cluster_half)
  int32_t N, C;
  int32_t* assign;       // [N]
  float* dist;           // [N] or NULL
};

// half[j] = |c_j|^2 / 2: summed in double in the order of the columns, rounded once
template <int D>
__global__ __launch_bounds__(256) void k_cluster_half(const float* cent, int C, float* half) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= C) return;
  const f32x4* row = (const f32x4*)(cent + (size_t)j * D);
  double s = 0.0;
  for (int c = 0; c < D / 4; ++c) {
    const f32x4 v = row[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)v[e] * (double)v[e];
  }
  half[j] = (float)(0.5 * s);
}

// the better of two (value, centroid) candidates of a row: the higher value, an equal one of the lower centroid (a NaN
// value never wins: both comparisons are false)
__device__ __forceinline__ void assign_take(float& bv, int& bj, float v, int j) {
  if (v > bv || (v == bv && j < bj)) {
    bv = v;
    bj = j;
  }
}

// A workgroup of 4 wavefronts takes 64 rows, a wavefront 16 of them: lane (q, r) holds row r's columns 16 kc + 4 q .. + 3 as
// the A fragment and, of a tile, the values of rows 4 q + i (i = 0 .. 3) against the centroid of its column r.  A lane keeps
// the best of its own columns per row (ascending j, so a strict > keeps the lower of equals), the 16 lanes of a q fold theirs.
// The start (-inf, centroid 0) is what a row whose values are all NaN ends with.
template <int D>
__global__ __launch_bounds__(256) void k_cluster_assign(AssignArgs a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int n0 = (blockIdx.x * 4 + wave) * 16;
  if (n0 >= a.N) return;                               // (uniform in the wavefront; no barrier below)
  const int row = n0 + r;
  f32x4 af[D / 16];
  double xx = 0.0;                                     // the lane's share of |x_row|^2
#pragma unroll
  for (int kc = 0; kc < D / 16; ++kc) {
    af[kc] = row < a.N ? *(const f32x4*)(a.x + (size_t)row * D + 16 * kc + 4 * q) : (f32x4)(0.0f);
#pragma unroll
    for (int e = 0; e < 4; ++e) xx += (double)af[kc][e] * (double)af[kc][e];
  }
  float bv[4];
  int bj[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bv[i] = -__builtin_inff();
    bj[i] = 0;
  }
  for (int c0 = 0; c0 < a.C; c0 += 64) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int j = c0 + 16 * tt + r;
      if (c0 + 16 * tt >= a.C) break;                  // (uniform)
      const int jc = min(j, a.C - 1);
      const f32x4 acc = score_tile_dense<D>(a.cent, af, jc, q);
      const float h = a.half[jc];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = acc[i] - h;
        if (j < a.C && v > bv[i]) {
          bv[i] = v;
          bj[i] = j;
        }
      }
    }
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {                   // (the 16 lanes of a q: xor of the low four lane bits)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ov = __shfl_xor(bv[i], m);
      const int oj = __shfl_xor(bj[i], m);
      assign_take(bv[i], bj[i], ov, oj);
    }
  }
  xx += __shfl_xor(xx, 16);                            // (one order for every lane: (q ^ 1) then (q ^ 2))
  xx += __shfl_xor(xx, 32);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double xr = __shfl(xx, 4 * q + i);           // row 4 q + i's norm sits in the lanes with r = 4 q + i
    const int out = n0 + 4 * q + i;
    if (r == 0 && out < a.N) {
      a.assign[out] = bj[i];
      if (a.dist) a.dist[out] = (float)fmax(xr - 2.0 * (double)bv[i], 0.0);
    }
  }
}

// Workgroup j sums the rows x[order[p]], p = seg_off[j] .. seg_off[j + 1] - 1, one column per thread, in double and in
// that order, and rounds the mean once.  An empty segment writes nothing.  Positions outside [0, N) and rows outside
// [0, N) are passed over (the caller's arrays are never trusted with an address).
template <int D>
__global__ __launch_bounds__(D) void k_cluster_means(const float* x, int N, const int32_t* order, const int32_t* seg_off,
                                                     float* cent) {
  const int j = blockIdx.x, c = threadIdx.x;
  const int lo = max(seg_off[j], 0), hi = min(seg_off[j + 1], N);
  double s = 0.0;
  int n = 0;
  for (int p = lo; p < hi; ++p) {
    const int row = order[p];
    if ((unsigned)row >= (unsigned)N) continue;        // (uniform: every thread reads the same entry)
    s += (double)x[(size_t)row * D + c];
    ++n;
  }
  if (n > 0) cent[(size_t)j * D + c] = (float)(s / (double)n);
}

struct ProbeArgs {
  TopkArgs t;                 // e.u_t = q, e.B = B, e.all_emb = cent, e.I = C, ids 1 : 1; K = P; ids = row_lists, scores in the workspace
  const float* scale;         // [C] or NULL (1)
  const float* bias;          // [C] or NULL (0)
  const int32_t* list_off;    // [C + 1] or NULL (every list counts)
};

// topk_scan's policy of the probe: score = fl(fl(v * scale_j) + bias_j), eval_score's two roundings; a list that list_off
// shows empty is never selected.
struct ProbeScore {
  const ProbeArgs& a;
  float sc, bias;
  bool full;
  f32x4 acc;
  __device__ __forceinline__ explicit ProbeScore(const ProbeArgs& a_) : a(a_) {}
  __device__ __forceinline__ bool row(int, int u) { return u < a.t.e.B; }
  __device__ __forceinline__ void col(const f32x4& tile, int j) {
    acc = tile;
    sc = a.scale ? a.scale[j] : 1.0f;
    bias = a.bias ? a.bias[j] : 0.0f;
    full = a.list_off ? a.list_off[j + 1] > a.list_off[j] : true;
  }
  __device__ __forceinline__ float score(int i) const { return eval_score(acc[i], sc, bias); }
  __device__ __forceinline__ bool may(int, int) const { return full; }
};

// grid (ceil(B / 16), 1): one slice, so the kept lists are the rows' results (row_lists [B, 1, P]; key 0 leaves -1)
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, 2) void k_cluster_probe(ProbeArgs pa) {
  __shared__ TopkSmem<KP, BUF> sm;
  ProbeScore pol(pa);
  topk_scan<D, KP, BUF, true>(sm, pa.t, pol, AllItems());
}

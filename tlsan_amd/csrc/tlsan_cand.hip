// Candidate scoring, candidate ranks and negative sampling (tlsan_cand.h): the instantiations and their launches.
// Arguments are checked by the callers in tlsan_api_eval.hip (tlsan_score_candidates, tlsan_candidate_ranks,
// tlsan_sample_negatives, tlsan_eval_ranks_excl / tlsan_eval_counts_shard_excl).
#include "tlsan_cand.h"

// One wavefront per row, four rows per workgroup.  Candidates with a negative id and repeats of candidate 0's id are
// not counted.
__global__ __launch_bounds__(256) void k_cand_ranks(const int32_t* cand, const float* scores, int B, int C,
                                                    int32_t* ranks) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int32_t* crow = cand + (size_t)b * C;
  const float* srow = scores + (size_t)b * C;
  const int id0 = crow[0];
  const topk_key_t k0 = topk_key(srow[0], id0);
  int cnt = 0;
  for (int c = 1 + lane; c < C; c += 64) {
    const int id = crow[c];
    if (id >= 0 && id != id0 && topk_key(srow[c], id) > k0) ++cnt;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) ranks[b] = cnt;
}

// One wavefront (workgroup) per row.  Round k draws t = 64 k + lane; a lane is accepted when its item is eligible, not
// in the row's set, and not the item of a lower lane of the round; the accepted lanes take the next slots in lane
// order (ballot prefix).  Stops at N accepted or 64 N draws.
__global__ __launch_bounds__(64) void k_sample_neg(NegArgs na) {
  __shared__ int set[NEG_HASH];
  const int lane = threadIdx.x, b = blockIdx.x;
  for (int i = lane; i < NEG_HASH; i += 64) set[i] = -1;
  const int N = na.N;
  int32_t* orow = na.out + (size_t)b * N;
  const int label = na.labels[b];
  const int xlo = na.excl_off ? na.excl_off[b] : 0, xhi = na.excl_off ? na.excl_off[b + 1] : 0;
  const uint64_t h = splitmix64(na.seed ^ (uint64_t)(na.row0 + b));
  const int64_t tmax = 64 * (int64_t)N;
  int cnt = 0;
  __syncthreads();
  for (int64_t t0 = 0; t0 < tmax && cnt < N; t0 += 64) {
    const int item = cand_draw(h, (uint64_t)(t0 + lane), na.item_count);
    bool ok = item != label && !topk_in_list(na.excl_ids, xlo, xhi, item);
    for (int j = 0; j < 64; ++j) {    // (uniform loop: every lane takes part in the shuffle)
      const int other = __shfl(item, j);
      if (j < lane && other == item) ok = false;
    }
    if (ok) {
      for (unsigned s = neg_slot(item);; s = (s + 1) & (NEG_HASH - 1)) {
        const int v = set[s];
        if (v == item) { ok = false; break; }
        if (v < 0) break;
      }
    }
    const unsigned long long m = __ballot(ok);
    const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                  // (every lookup of this round before the inserts)
    if (ok && pos < N) {
      orow[pos] = item;
      // (distinct items: a lost race moves on to the next slot)
      for (unsigned s = neg_slot(item);; s = (s + 1) & (NEG_HASH - 1))
        if (atomicCAS(&set[s], -1, item) == -1) break;
    }
    cnt += __popcll(m);
    __syncthreads();
  }
  for (int i = cnt + lane; i < N; i += 64) orow[i] = -1;
}

// The items of the rows' exclusion lists against the labels, in k_score_cand's layout: a wavefront holds the A fragments
// of 16 rows, column r of a tile is row r's e-th list entry, and the diagonal lane (row r, column r) takes the rank
// kernel's decision for it.  The 16x16 tile is the rank kernels' MFMA chain on the same operand values (the dense
// matrix where the rank path built one -- it holds the tables' stored values -- else the tables), and the last two
// operations are the score helper that kernel calls (ExclArgs.fused), so the decision is the counting kernel's bit for bit.
// grid (ceil(B/16), slices); wavefront w of slice y takes the entries e = (y * 4 + w) + k * 4 * slices.
template <int D>
__global__ __launch_bounds__(256) void k_excl_ahead(ExclArgs xa) {
  const EvalArgs& a = xa.e;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * 16, u = u0 + r;
  const bool uv = u < a.B;
  const int lo = uv ? xa.excl_off[u] : 0;
  int len = uv ? xa.excl_off[u + 1] - lo : 0;
  {  // ids past the table's last one are never held, and the list ascends: leave its tail out (lists often come as
     // slots of one width padded with such ids)
    const int gmax = (a.I - 1) * a.id_mul + a.id_add;
    int l = 0, h = len;
    while (l < h) {
      const int m = (l + h) >> 1;
      if (xa.excl_ids[lo + m] > gmax) h = m; else l = m + 1;
    }
    len = l;
  }
  int lmax = len;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) lmax = max(lmax, __shfl_xor(lmax, o));   // (the tile's longest list: a uniform loop)
  const int e0 = blockIdx.y * 4 + wave;
  if (e0 >= lmax) return;
  f32x4 af[D / 16];
  load_user_frag<D>(a, u0, q, r, af);
  const float P = eval_scale(a);
  const int lab = uv ? a.labels[u] : -1;
  const float sl = uv ? a.s_label[u] : 0.0f;
  const bool diag = uv && q == (r >> 2);
  int n_ahead = 0, n_held = 0;
  for (int e = e0; e < lmax; e += gridDim.y * 4) {
    int g = -1, n = -1;
    if (e < len) {
      g = xa.excl_ids[lo + e];
      const bool first = e == 0 || xa.excl_ids[lo + e - 1] != g;
      n = (first && g != lab) ? cand_local(g, a.I, a.id_mul, a.id_add) : -1;
    }
    const int item = n >= 0 ? n : 0;
    const f32x4 acc = a.all_emb ? score_tile_dense<D>(a.all_emb, af, item, q) : score_tile<D>(a, af, item, q);
    const float bias = a.p.item_b[(size_t)item * a.p.ld_itemb];
    if (diag && n >= 0) {
      const float v = tile_diag(acc, r);
      const float s = xa.fused ? eval_score_fma(v, P, bias) : eval_score(v, P, bias);
      n_held += 1;
      n_ahead += rank_ahead(s, sl, g, lab) ? 1 : 0;   // (g != lab: such an entry has n < 0)
    }
  }
  if (diag) {
    if (n_held) atomicAdd(&xa.held[u], n_held);
    if (n_ahead) atomicAdd(&xa.ahead[u], n_ahead);
  }
}

hipError_t tlsan_launch_excl_ahead(const ExclArgs& a, int D, hipStream_t hs) {
  const int ut = (a.e.B + 15) / 16;
  // (at most 64 slices: a wavefront whose first entry lies past its tile's longest list leaves at once)
  const dim3 grid(ut, eval_slices(ut, 64));
  dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(k_excl_ahead<d.value>, grid, dim3(256), 0, hs, a); });
  return hipGetLastError();
}

hipError_t tlsan_launch_score_cand(const CandArgs& a, int D, hipStream_t hs) {
  const int ut = (a.e.B + 15) / 16;
  const dim3 grid(ut, eval_slices(ut, (a.C + 3) / 4));
  dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(k_score_cand<d.value>, grid, dim3(256), 0, hs, a); });
  return hipGetLastError();
}

hipError_t tlsan_launch_cand_ranks(const int32_t* cand, const float* scores, int B, int C, int32_t* ranks,
                                   hipStream_t hs) {
  hipLaunchKernelGGL(k_cand_ranks, dim3((B + 3) / 4), dim3(256), 0, hs, cand, scores, B, C, ranks);
  return hipGetLastError();
}

hipError_t tlsan_launch_sample_neg(const NegArgs& a, hipStream_t hs) {
  hipLaunchKernelGGL(k_sample_neg, dim3(a.B), dim3(64), 0, hs, a);
  return hipGetLastError();
}

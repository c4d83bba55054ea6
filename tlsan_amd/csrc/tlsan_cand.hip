// Candidate scoring, candidate ranks and negative sampling (tlsan_cand.h): the instantiations and their launches.
// Arguments are checked by the callers in tlsan_api.hip (tlsan_score_candidates, tlsan_candidate_ranks,
// tlsan_sample_negatives).
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

hipError_t tlsan_launch_score_cand(const CandArgs& a, int D, hipStream_t hs) {
  const int ut = (a.e.B + 15) / 16;
  const int want = (2048 + ut - 1) / ut;  // enough workgroups to fill the chip (the rank path's slicing)
  int nsl = (a.C + 3) / 4;
  if (nsl > want) nsl = want;
  if (nsl < 1) nsl = 1;
  const dim3 grid(ut, nsl);
  if (D == 64) hipLaunchKernelGGL(k_score_cand<64>, grid, dim3(256), 0, hs, a);
  else if (D == 128) hipLaunchKernelGGL(k_score_cand<128>, grid, dim3(256), 0, hs, a);
  else hipLaunchKernelGGL(k_score_cand<256>, grid, dim3(256), 0, hs, a);
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

// tlsan_cand.h -- scores of caller-given candidate items, their ranks, and the sampled-negatives evaluation.
//
// k_score_cand: scores[b, c] = u_t[b] . [item_emb || cate_emb[item_cate]][g] * P + item_b[g] for g = cand[b, c], in the
// form of k_eval_label: a wavefront holds the A fragments of 16 rows (load_user_frag) and, for each candidate column
// c, scores one 16x16 tile whose lane column r is row r's candidate (score_tile) and keeps the diagonal (tile_diag).  The
// diagonal element is the same MFMA chain on the same operands as the label's own score, and the two roundings (* P,
// + bias) are kept apart (eval_score), so a candidate's score equals tlsan_eval_label_scores' (and a tlsan_eval_topk list entry's) bit for
// bit.  One MFMA column in 16 is kept; the kernel is bound by the row gathers, not by the matrix pipe.
//
// k_cand_ranks (tlsan_cand.hip): how many candidates c >= 1 of a row come ahead of candidate 0, in tf.nn.top_k's
// order (topk_key).
//
// k_sample_neg (tlsan_cand.hip): the first N distinct eligible items of the row's draw sequence (cand_draw); the
// definition is in include/tlsan.h.
//
// k_excl_ahead (tlsan_cand.hip): for the items of a row's exclusion list, the decision the all-items rank kernel took
// for them (ExclArgs below) -- what a filtered rank subtracts from tlsan_eval_ranks' rank.
#pragma once
#include "tlsan_eval.h"
#include "tlsan_topk.h"

#define NEG_MAX 1024

struct CandArgs {
  EvalArgs e;               // scoring: p, u_t, B, I, di, dc, id_mul, id_add (labels, s_label, ranks, all_emb unused)
  int32_t C;
  const int32_t* cand;      // [B, C] global item ids
  float* scores;            // [B, C]
};

// k_excl_ahead: row b's list is excl_ids[excl_off[b] .. excl_off[b + 1]) (global ids, ascending).  An entry counts when
// it is the first of its value, is not the row's label and is held by this table (cand_local); held[b] += 1 for it, and
// ahead[b] += 1 when the rank kernel of this table counted it ahead of the label.  `fused` says which rank kernel that
// was, by the score form it calls (tlsan_eval.h): k_eval_rank_dense (e.all_emb set) eval_score_fma, one fused
// multiply-add; k_eval_rank eval_score, a rounded product and a rounded sum.  k_excl_ahead calls the same helper.
struct ExclArgs {
  EvalArgs e;               // p, u_t, labels (global ids), s_label, B, I, di, dc, all_emb (dense form), id_mul, id_add
  const int32_t* excl_off;  // [B + 1]
  const int32_t* excl_ids;
  int32_t* ahead;           // [B], zeroed before the launch
  int32_t* held;            // [B], zeroed before the launch
  int32_t fused;            // 1: eval_score_fma (k_eval_rank_dense); 0: eval_score (k_eval_rank)
};

// Local item of global id g, or -1 when this table does not hold it.
__device__ __forceinline__ int cand_local(int g, int I, int id_mul, int id_add) {
  if (g < id_add) return -1;
  const int o = g - id_add;
  const int n = id_mul == 1 ? o : o / id_mul;
  return (n * id_mul == o && n < I) ? n : -1;
}

// grid (ceil(B/16), slices); wavefront w of slice y scores columns c = (y * 4 + w) + k * 4 * slices.
template <int D>
__global__ __launch_bounds__(256) void k_score_cand(CandArgs ca) {
  const EvalArgs& a = ca.e;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * 16, u = u0 + r;
  const bool uv = u < a.B;
  const bool whole = a.id_mul == 1 && a.id_add == 0;   // whole table: ids outside it score -inf (else: not ours, skipped)
  f32x4 af[D / 16];
  load_user_frag<D>(a, u0, q, r, af);
  const float P = eval_scale(a);
  const int32_t* crow = ca.cand + (size_t)(uv ? u : 0) * ca.C;
  float* srow = ca.scores + (size_t)(uv ? u : 0) * ca.C;
  for (int c = blockIdx.y * 4 + wave; c < ca.C; c += gridDim.y * 4) {
    const int n = uv ? cand_local(crow[c], a.I, a.id_mul, a.id_add) : -1;
    const int item = n >= 0 ? n : 0;
    // (two roundings, as k_eval_label forms the label's score)
    const f32x4 s = eval_score(score_tile<D>(a, af, item, q), P, a.p.item_b[(size_t)item * a.p.ld_itemb]);
    if (uv && q == (r >> 2)) {   // the diagonal: row r's candidate
      if (n >= 0) srow[c] = tile_diag(s, r);
      else if (whole) srow[c] = -__builtin_inff();
    }
  }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// item of draw t of a row whose stream is h = splitmix64(seed ^ row)
__device__ __forceinline__ int cand_draw(uint64_t h, uint64_t t, int item_count) {
  const uint64_t key = splitmix64(h ^ t);
  return (int)(((key >> 32) * (uint64_t)item_count) >> 32);
}

#define NEG_HASH (2 * NEG_MAX)   // LDS open-addressing set of the row's accepted items (load <= 1/2)

struct NegArgs {
  int32_t item_count, B, N;
  uint64_t seed;
  int64_t row0;
  const int32_t* labels;    // [B]
  const int32_t* excl_off;  // [B + 1] or NULL
  const int32_t* excl_ids;
  int32_t* out;             // [B, N]
};

__device__ __forceinline__ unsigned neg_slot(int item) { return ((unsigned)item * 2654435761u) >> 21; }  // 11 bits

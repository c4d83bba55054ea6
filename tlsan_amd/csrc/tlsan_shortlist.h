// tlsan_shortlist.h -- the bf16 shortlist index: an exact top-K over all items in two stages, with a per-row certificate.
//
// Stage 1 (k_shortlist_topk) selects, per row of u_t, the N items of highest APPROXIMATE score
//   a~(b, n) = fl(fl(acc~ * P) + item_b[n]),   acc~ = the fp32 accumulation by v_mfma_f32_16x16x32_bf16 of bf16(u_t[b]) . vec[n],
// over vec [I, d], the bf16 (round-to-nearest-even) snapshot of [item_emb || cate_emb[item_cate]] as stored that
// k_shortlist_build writes, in topk_key's order on (a~, global id).  Stage 2 scores the shortlist with the exact path's own
// scorer (tlsan_score_candidates) and k_shortlist_select picks each row's K best by exact key and decides, per row, whether
// the shortlist provably holds the exact top K of the whole table (include/tlsan.h: the certificate; DESIGN.md section 7: why
// it is sound).
//
// Why stage 1 is cheap where k_eval_topk is not: the bf16 matrix instruction contracts 32 k-slots where the exact fp32
// one contracts 4, a row of vec is half the bytes, and a wavefront holds the A fragments of T tiles of 16 rows (T * d/32 * 4
// registers) and issues T MFMAs per loaded item fragment: the table is read once per 16 T rows instead of once per 16.
// The C/D layout of the 16x16x32 form is the fp32 form's (lane (q, r): rows 4q .. 4q+3 of column r), so the keys, the
// exclusion lists, the offers and the slices' merge are k_eval_topk's, on one TopkSmem per row tile.
#pragma once
#include "tlsan_eval.h"
#include "tlsan_topk.h"

#define SHORTLIST_NMIN 16
#define SHORTLIST_NMAX TOPK_MAX

typedef __bf16 sl_bf16x8 __attribute__((ext_vector_type(8)));

// ---- the snapshot ---------------------------------------------------------------------------------------------------
struct ShortlistBuildArgs {
  EvalArgs e;          // p (tables as stored), I, di, dc -- read through all_emb4
  uint16_t* vec;       // [I, D] bf16
  uint32_t* wmax;      // the bit pattern of max_n ||w_n||_2, cleared before the launch
};

// four floats -> four bf16 (nearest even; a bf16 table's values are bf16 already and come through unchanged)
__device__ __forceinline__ uint2 sl_pack4(f32x4 v) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
  uint2 u;
  u.x = __builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2));
  u.y = __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2));
  return u;
}

// D / 8 lanes per item, 8 columns and one 16-byte store per lane.  The row's sum of squares: the lane's eight in column
// order, then the lanes' by a butterfly -- one order for a given D; the norm sqrtf of it.  The maximum over the items is an
// integer maximum on the bit patterns of the (non-negative) norms, which does not depend on the order the workgroups
// arrive in; a norm that is NaN or inf enters as +inf.
template <int D>
__global__ __launch_bounds__(256) void k_shortlist_build(ShortlistBuildArgs ba) {
  constexpr int LPI = D / 8;               // lanes per item (8, 16 or 32: a part of one wavefront)
  const EvalArgs& a = ba.e;
  const int t = threadIdx.x, j = t % LPI;
  const long long it0 = (long long)blockIdx.x * (256 / LPI) + t / LPI;
  const bool valid = it0 < a.I;
  const int it = valid ? (int)it0 : a.I - 1;
  const f32x4 v0 = all_emb4(a, it, 8 * j), v1 = all_emb4(a, it, 8 * j + 4);
  if (valid) {
    const uint2 p0 = sl_pack4(v0), p1 = sl_pack4(v1);
    *(uint4*)(ba.vec + (size_t)it * D + 8 * j) = make_uint4(p0.x, p0.y, p1.x, p1.y);
  }
  float ss = 0.0f;
#pragma unroll
  for (int s = 0; s < 4; ++s) ss = __builtin_fmaf(v0[s], v0[s], ss);
#pragma unroll
  for (int s = 0; s < 4; ++s) ss = __builtin_fmaf(v1[s], v1[s], ss);
#pragma unroll
  for (int o = 1; o < LPI; o <<= 1) ss += __shfl_xor(ss, o);
  float nrm = __builtin_sqrtf(ss);
  if (!(nrm < __builtin_inff())) nrm = __builtin_inff();
  uint32_t m = valid ? __float_as_uint(nrm) : 0u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((t & 63) == 0 && m != 0u) atomicMax(ba.wmax, m);
}

// ---- stage 1 --------------------------------------------------------------------------------------------------------
struct ShortlistArgs {
  const uint16_t* vec;        // [I, D] bf16
  const float* u_t;           // [B, D]
  const float* scale;         // P, or NULL (1)
  const float* item_b;        // item n's bias at item_b[n * ld_itemb]
  int32_t B, I, ld_itemb, N;
  int32_t id_mul, id_add;     // local item n is global id n * id_mul + id_add
  const int32_t* excl_off;    // [B + 1] / ascending global ids, topk_scan's format, or NULL
  const int32_t* excl_ids;
  int32_t* ids;               // [B, gridDim.y, N]
  float* approx;              // [B, gridDim.y, N]
};

// Row tiles of a workgroup: T TopkSmem of 18 / 24 / 64 KB in the 160 KB of LDS, and T * d/32 * 4 registers of A fragments
// and 4 T accumulators per lane.  Two everywhere: four fit the LDS for N <= 64, but with their accumulators, thresholds and
// keys the lane no longer fits 256 registers, and stage 1 measured 54.4 ms against 32.5 ms with two (5 M items, 4096 rows,
// d = 128, N = 64: profiles/shortlist.md).
constexpr int SHORTLIST_T = 2;

// grid (ceil(B / 16T), slices), 256 threads.  Wavefront w of slice y scores items n0 .. n0 + 63, n0 = (round * slices + y) *
// 256 + 64 w, as four item tiles; every loaded item fragment (16 bytes per lane: lane (q, r) holds k-slots 8q .. 8q+7 of
// the chunk of item r) feeds the MFMAs of all T row tiles.
template <int D, int KP, int BUF, int T>
__global__ __launch_bounds__(256) void k_shortlist_topk(ShortlistArgs a) {
  // (score = (acc * P) + bias in two roundings, as k_eval_topk)
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char sl_lds[];
  TopkSmem<KP, BUF>* sm = (TopkSmem<KP, BUF>*)sl_lds;
  constexpr int NC = D / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * (16 * T);
#pragma unroll
  for (int t = 0; t < T; ++t) topk_init(sm[t]);
  // A fragments: row u0 + 16 t + r, k-slots 32 kc + 8q .. + 7, rounded to bf16 once
  sl_bf16x8 af[T][NC];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int u = u0 + 16 * t + r;
#pragma unroll
    for (int kc = 0; kc < NC; ++kc) {
      f32x4 lo = (f32x4)(0.0f), hi = (f32x4)(0.0f);
      if (u < a.B) {
        const float* src = a.u_t + (size_t)u * D + 32 * kc + 8 * q;
        lo = *(const f32x4*)src;
        hi = *(const f32x4*)(src + 4);
      }
      const uint2 p0 = sl_pack4(lo), p1 = sl_pack4(hi);
      af[t][kc] = __builtin_bit_cast(sl_bf16x8, make_uint4(p0.x, p0.y, p1.x, p1.y));
    }
  }
  const float P = a.scale ? *a.scale : 1.0f;
  topk_key_t thr[T][4];
  float thrf[T][4];        // the score of the threshold key: a score below it cannot beat the key
  unsigned uvm = 0;        // bit 4 t + i: row u0 + 16 t + 4 q + i exists
  int ph[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    ph[t] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      thr[t][i] = 0ull;
      thrf[t][i] = -__builtin_inff();
      if (u0 + 16 * t + 4 * q + i < a.B) uvm |= 1u << (4 * t + i);
    }
  }
  __syncthreads();
  const int step = gridDim.y * 256;
  const int nround = (a.I + step - 1) / step;
  for (int rd = 0; rd < nround; ++rd) {
    const int n0 = rd * step + (blockIdx.y * 4 + wave) * 64;
    const bool live = n0 < a.I;
    f32x4 acc[T][4];
    int gn[4];
    float bias[4];
    unsigned vnm = 0;      // bit tt: the lane's column of item tile tt is an item
    if (live) {
      const uint16_t* rows[4];
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int n = n0 + 16 * tt + r;
        const int item = min(n, a.I - 1);
        if (n < a.I) vnm |= 1u << tt;
        gn[tt] = item * a.id_mul + a.id_add;
        rows[tt] = a.vec + (size_t)item * D + 8 * q;
        bias[tt] = a.item_b[(size_t)item * a.ld_itemb];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t][tt] = (f32x4)(0.0f);
      }
#pragma unroll
      for (int kc = 0; kc < NC; ++kc) {
        sl_bf16x8 bv[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) bv[tt] = __builtin_bit_cast(sl_bf16x8, *(const uint4*)(rows[tt] + 32 * kc));
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int tt = 0; tt < 4; ++tt)
            acc[t][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t][kc], bv[tt], acc[t][tt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      topk_key_t key[16];
      unsigned pend = 0;
      if (live) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const f32x4 sc = acc[t][tt] * P;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float s = sc[i] + bias[tt];
            key[4 * tt + i] = 0ull;
            // one float compare rejects most scores before a key is formed; what passes is decided on the keys, and
            // the exclusion list is searched only for those
            if (s < thrf[t][i] || !(vnm & (1u << tt)) || !(uvm & (1u << (4 * t + i)))) continue;
            const topk_key_t k = topk_key(s, gn[tt]);
            key[4 * tt + i] = k;
            if (k <= thr[t][i]) continue;
            if (a.excl_off) {
              const int u = u0 + 16 * t + 4 * q + i;
              if (topk_in_list(a.excl_ids, a.excl_off[u], a.excl_off[u + 1], gn[tt])) continue;
            }
            pend |= 1u << (4 * tt + i);
          }
        }
      }
      topk_offer(sm[t], key, pend, 4 * q, thr[t], a.N, ph[t]);
#pragma unroll
      for (int i = 0; i < 4; ++i) thrf[t][i] = topk_key_score(thr[t][i]);
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) topk_finish(sm[t], u0 + 16 * t, a.B, a.N, gridDim.y, blockIdx.y, a.ids, a.approx);
}

// ---- stage 2: select by exact key, certify ----------------------------------------------------------------------------
// c of the certificate: 2^-7 + 2^-11 (DESIGN.md section 7 derives it; it is not a tuning knob)
#define SHORTLIST_C (0.0078125 + 0.00048828125)

struct ShortlistSelArgs {
  const int32_t* sl_ids;     // [B, N] stage 1's shortlist (global ids, -1 padding at the end)
  const float* sl_exact;     // [B, N] tlsan_score_candidates' scores of it
  const float* sl_approx;    // [B, N] stage 1's scores
  const float* u_t;          // [B, D]
  const float* scale;        // P or NULL
  const float* wmax;         // the snapshot's norm bound
  int32_t B, N, K;
  int32_t* ids;              // [B, K]
  float* scores;             // [B, K]
  int32_t* certified;        // [B]
};

__device__ __forceinline__ bool sl_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// 16 rows per workgroup, 16 threads per row (k_topk_merge's shape); a round offers 64 entries of every row.
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256) void k_shortlist_select(ShortlistSelArgs a) {
  __shared__ TopkSmem<KP, BUF> sm;
  const int u = threadIdx.x >> 4, c0 = threadIdx.x & 15;
  const int u0 = blockIdx.x * 16, row = u0 + u;
  const bool rv = row < a.B;
  topk_init(sm);
  // ||u_t[row]||_2 in fp32: the thread's D / 16 columns c0, c0 + 16, .. in order, then the 16 threads' by a butterfly
  float ss = 0.0f;
  if (rv) {
#pragma unroll
    for (int c = 0; c < D / 16; ++c) {
      const float x = a.u_t[(size_t)row * D + 16 * c + c0];
      ss = __builtin_fmaf(x, x, ss);
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o);
  __syncthreads();
  const int nround = (a.N + 63) / 64;
  topk_key_t thr[1] = {0ull};
  int ph = 0;
  for (int rd = 0; rd < nround; ++rd) {
    topk_key_t key[4];
    unsigned pend = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = rd * 64 + 16 * j + c0;
      key[j] = 0ull;
      if (rv && e < a.N) {
        const size_t o = (size_t)row * a.N + e;
        const int id = a.sl_ids[o];
        if (id >= 0) key[j] = topk_key(a.sl_exact[o], id);
      }
      if (key[j] > thr[0]) pend |= 1u << j;
    }
    topk_offer(sm, key, pend, u, thr, a.K, ph);
  }
  topk_finish(sm, u0, a.B, a.K, 1, 0, a.ids, a.scores);
  if (rv && c0 == 0) {
    const size_t last = (size_t)row * a.N + (a.N - 1);
    int cert;
    if (a.sl_ids[last] < 0) {
      cert = 1;   // fewer than N eligible items: all of them are in the shortlist
    } else {
      const double sK = (double)topk_key_score(sm.kept[u][a.K - 1]), aN = (double)a.sl_approx[last];
      const double P = a.scale ? (double)*a.scale : 1.0;
      const double eps = SHORTLIST_C * __builtin_fabs(P) * (double)__builtin_sqrtf(ss) * (double)*a.wmax +
                         0x1p-20 * (__builtin_fabs(sK) + __builtin_fabs(aN));
      cert = (sl_finite(sK) && sl_finite(aN) && sl_finite(eps) && sK > aN + eps) ? 1 : 0;
    }
    a.certified[row] = cert;
  }
}

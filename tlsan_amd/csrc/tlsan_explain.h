// tlsan_explain.h -- explanations: the exact per-source parts of a listed score (include/tlsan.h, tlsan_explain).
//
// k_explain: one workgroup takes row b and a tile of up to T items (T = 16, 32 or 64, the launcher's choice).  In LDS it
// holds the tile's item vectors w [T, D] (true values: P * stored), the bridge vectors v [T, D] and the tile's parts
// pt [T, R]; nothing of size [B, Kc, R] exists unless the caller asks for `parts`.
//   1. setup: the row's bridge attention a1[b, 0, :], its user vector, a1[b, 0, :] o k0, the ids and scales of its
//      positions, the item rows w;
//   2. v = K (a1[b, 0, :] o w) for the whole tile on v_mfma_f32_16x16x4_f32: the tile's items are the M rows, K (shared by
//      every row of the launch, read through the caches) the B operand.  Wavefront w owns the output columns
//      [w D/4, (w + 1) D/4): D / 64 independent accumulators per 16 items, so the chains of one accumulator (40 cycles
//      dependent latency against 32 of issue) overlap;
//   3. the parts: a wavefront takes a source vector -- the user vector, a1_0 o k0, a long-term position's
//      a0[b, l, :] o h[b, l, :] or a session position's a1[b, 1 + j, :] o h_new[b, j, :] --, lays it into its own LDS row and
//      dots it with 16 items' w (user, offset, session) or v (long-term) at a time: four lanes per item, each over the
//      channels c = lane & 3 (mod 4) -- conflict-free reads of rows D + 4 apart --, two butterfly steps.  Positions past the
//      row's lengths and padding items get 0.0f whatever the arithmetic gave;
//   4. `parts` is written from LDS when asked for;
//   5. by item: a source's value replaces its leader's part in LDS (its members summed in ascending column order);
//   6. the selection: a thread per (item, source) counts the sources of its item that come before its own under
//      explain_better -- a strict total order, so the counts are the ranks -- and writes its own when the rank is below r;
//      the places past the row's sources get the empty pattern.  No cross-lane step.
// The selection reads the LDS values that step 4 writes, so top_* is the selection over `parts` bit for bit, with or
// without `parts`.
#pragma once
#include "tlsan_common.h"

#define EXPLAIN_TMAX 64          // items of a tile
#define EXPLAIN_WPAD 4           // floats between the LDS rows of w and v (a tile row's 16-B pieces land on distinct banks)
// positions of a row, Ls + Sn: the longest window and the longest session the training step takes (TLSAN_LS_CAP +
// TLSAN_SN_CAP).  The leader search costs Rh^2 / 2 compares per workgroup and the selection T * Rh^2: quadratic in the row's
// positions, 9 216 compares per thread at the cap with 64 items.
#define EXPLAIN_RH_MAX (TLSAN_LS_CAP + TLSAN_SN_CAP)
#define EXPLAIN_LDS_MAX (160 * 1024)

struct ExplainArgs {
  tlsan_params p;           // strides filled in (norm_params)
  int32_t B, Sn, Ls, dh, di, dc, Kc;
  int32_t T, RS;            // items of a tile (16, 32, 64); floats between the LDS rows of the parts (>= R)
  int32_t r, by, order;
  int32_t oK, ok0, ogamma;  // offsets into p.dense
  const int32_t *u, *hist_i, *hist_i_new, *sl, *sl_new, *u_cate;
  const float* hist_t;
  const float *att0, *att1;
  const int32_t* items;     // [B, Kc]
  float* parts;             // [B, Kc, R] or NULL
  int32_t *top_src, *top_item;   // [B, Kc, r] or NULL (together with top_val)
  float* top_val;
};

// The carve-up of the workgroup's dynamic LDS, in floats: one definition for the kernel and the launcher.
struct ExplainLds { int w, v, pt, a10, ue, k0a, xs, psc, ids, pid, lead, nsrc, total; };
__host__ __device__ inline ExplainLds explain_lds(int D, int T, int RS, int Ls, int Rh) {
  ExplainLds o;
  int n = 0;
  o.w = n; n += T * (D + EXPLAIN_WPAD);
  o.v = n; n += T * (D + EXPLAIN_WPAD);
  o.pt = n; n += T * RS;            // (T is a multiple of 16: what follows stays 16-B aligned)
  o.a10 = n; n += D;
  o.ue = n; n += D;
  o.k0a = n; n += D;
  o.xs = n; n += 4 * D;             // a source vector per wavefront
  o.psc = n; n += Ls;
  o.ids = n; n += T;
  o.pid = n; n += Rh;
  o.lead = n; n += Rh;
  o.nsrc = n; n += 1;
  o.total = n;
  return o;
}

template <int DT>
__device__ __forceinline__ float tbl_ld1(const float* __restrict__ base, size_t idx) {
  if constexpr (DT == TLSAN_TABLE_F32) return base[idx];
  else return __uint_as_float((uint32_t)((const uint16_t*)base)[idx] << 16);
}

// element c of the stored vector [item_emb[g] || cate_emb[item_cate[g]]]
template <int DT>
__device__ __forceinline__ float explain_item1(const ExplainArgs& a, int g, int c) {
  return c < a.di ? tbl_ld1<DT>(a.p.item_emb, (size_t)g * a.p.ld_item + c)
                  : tbl_ld1<DT>(a.p.cate_emb, (size_t)a.p.item_cate[g] * a.dc + (c - a.di));
}

// Source (va, position pa) comes before (vb, pb), pa != pb: a NaN loses to every number; the larger key (the value, or its
// magnitude) wins; equal keys and two NaNs go to the lower position.  A strict total order of an item's sources.
__device__ __forceinline__ bool explain_better(float va, int pa, float vb, int pb, int order) {
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return nb;
  if (!na) {
    const float ka = order == TLSAN_EXPLAIN_ABS ? __builtin_fabsf(va) : va;
    const float kb = order == TLSAN_EXPLAIN_ABS ? __builtin_fabsf(vb) : vb;
    if (ka != kb) return ka > kb;
  }
  return pa < pb;
}

// grid: B * ceil(Kc / T) workgroups of 256 threads; dynamic LDS: explain_lds(...).total floats
template <int D, int DT>
__global__ __launch_bounds__(256) void k_explain(ExplainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, r16 = lane & 15;
  const int ntile = (a.Kc + a.T - 1) / a.T;
  const int b = blockIdx.x / ntile, t0 = (blockIdx.x % ntile) * a.T;
  const int Ta = min(a.T, (a.Kc - t0 + 15) & ~15);     // the tile's rows in use, whole 16-row MFMA tiles
  const int Ls = a.Ls, Sn = a.Sn, Rh = Ls + Sn, R = 3 + Rh, RS = a.RS, dh = a.dh;
  constexpr int WS = D + EXPLAIN_WPAD;
  const ExplainLds o = explain_lds(D, a.T, RS, Ls, Rh);
  float* w = smem + o.w;
  float* v = smem + o.v;
  float* pt = smem + o.pt;
  float* a10 = smem + o.a10;
  float* ue = smem + o.ue;
  float* k0a = smem + o.k0a;
  float* psc = smem + o.psc;
  int* ids = (int*)(smem + o.ids);
  int* pid = (int*)(smem + o.pid);
  int* lead = (int*)(smem + o.lead);
  int* nsrc = (int*)(smem + o.nsrc);
  const float P = a.p.scale ? *a.p.scale : 1.0f;
  const size_t a1row = (size_t)(1 + Sn) * dh, a0row = (size_t)Ls * dh;   // floats of one (head, sample) block

  // ---- 1. setup
  {
    const int u = a.u[b], uc = a.u_cate[b];
    for (int c = tid; c < D; c += 256) {
      const float x = a.att1[((size_t)(c / dh) * a.B + b) * a1row + (c % dh)];
      a10[c] = x;
      k0a[c] = x * a.p.dense[a.ok0 + c];
      ue[c] = P * (c < a.di ? tbl_ld1<DT>(a.p.user_emb, (size_t)u * a.p.ld_user + c)
                            : tbl_ld1<DT>(a.p.cate_emb, (size_t)uc * a.dc + (c - a.di)));
    }
    const int sl = a.sl[b], sln = a.sl_new[b];
    const float gamma = a.p.dense[a.ogamma];
    for (int p = tid; p < Rh; p += 256) {
      if (p < Ls) {
        pid[p] = p < sl ? a.hist_i[(size_t)b * Ls + p] : -1;
        psc[p] = gamma * (P * a.p.usert_emb[(size_t)u * a.p.ld_usert + p]) * a.hist_t[(size_t)b * Ls + p];
      } else {
        pid[p] = (p - Ls) < sln ? a.hist_i_new[(size_t)b * Sn + (p - Ls)] : -1;
      }
    }
    for (int t = tid; t < a.T; t += 256) ids[t] = (t0 + t) < a.Kc ? a.items[(size_t)b * a.Kc + t0 + t] : -1;
    if (tid == 0) *nsrc = 0;
  }
  __syncthreads();
  for (int p = tid; p < Rh; p += 256) {     // the lowest valid position that holds the same item id (-1: not valid)
    const int id = pid[p];
    int l = -1;
    if (id >= 0) {
      l = p;
      for (int k = 0; k < p; ++k)
        if (pid[k] == id) { l = k; break; }
    }
    lead[p] = l;
    if (a.by == TLSAN_EXPLAIN_BY_ITEM ? l == p : l >= 0) atomicAdd(nsrc, 1);     // (the row's sources)
  }
  for (int e = tid; e < Ta * (D / 4); e += 256) {
    const int t = e / (D / 4), c = 4 * (e % (D / 4));
    const int g = ids[t];
    f32x4 x = (f32x4)(0.0f);
    if (g >= 0) {
      x = c < a.di ? tbl_ld4<DT>(a.p.item_emb, (size_t)g * a.p.ld_item + c)
                   : tbl_ld4<DT>(a.p.cate_emb, (size_t)a.p.item_cate[g] * a.dc + (c - a.di));
      x *= P;
    }
    *(f32x4*)(w + t * WS + c) = x;
  }
  for (int t = tid; t < Ta; t += 256) pt[t * RS] = ids[t] >= 0 ? a.p.item_b[(size_t)ids[t] * a.p.ld_itemb] : 0.0f;
  __syncthreads();

  // ---- 2. v[t, c'] = sum_c K[c', c] a10[c] w[t, c]: lane (r16, q) supplies k = 16 kc + 4 q + s of both operands
  {
    constexpr int NT = D / 64;
    const int MS = Ta / 16;
    const float* Kp = a.p.dense + a.oK;
    f32x4 acc[4][NT];
#pragma unroll
    for (int ms = 0; ms < 4; ++ms)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[ms][j] = (f32x4)(0.0f);
#pragma unroll 2
    for (int kc = 0; kc < D / 16; ++kc) {
      f32x4 bv[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bv[j] = *(const f32x4*)(Kp + (size_t)((wave * NT + j) * 16 + r16) * D + 16 * kc + 4 * q);
      const f32x4 s4 = *(const f32x4*)(a10 + 16 * kc + 4 * q);
#pragma unroll
      for (int ms = 0; ms < 4; ++ms) {
        if (ms < MS) {
          const f32x4 av = *(const f32x4*)(w + (ms * 16 + r16) * WS + 16 * kc + 4 * q) * s4;
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[ms][j] = TLSAN_MFMA(av[s], bv[j][s], acc[ms][j]);
        }
      }
    }
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      if (ms < MS) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) v[(ms * 16 + 4 * q + i) * WS + (wave * NT + j) * 16 + r16] = acc[ms][j][i];
      }
    }
  }
  __syncthreads();

  // ---- 3. the parts: source pp = 0 user, 1 bridge offset, 2 + p position p
  {
    float* xs = smem + o.xs + wave * D;
    const int seg = lane & 3;
    for (int pp = wave; pp < Rh + 2; pp += 4) {
      const float* base = w;
      const float* sv = pp == 0 ? ue : k0a;
      const int col = 1 + pp;
      bool valid = true;
      if (pp >= 2) {
        const int p = pp - 2, id = pid[p];
        valid = id >= 0;
        sv = xs;
        wave_lds_fence();          // (the last source's reads before its row is overwritten)
        if (valid) {
          if (p < Ls) {
            base = v;
            const float sc = psc[p];
#pragma unroll
            for (int i = 0; i < D / 64; ++i) {
              const int c = lane + 64 * i;
              xs[c] = a.att0[((size_t)(c / dh) * a.B + b) * a0row + (size_t)p * dh + (c % dh)] * (P * explain_item1<DT>(a, id, c)) * sc;
            }
          } else {
#pragma unroll
            for (int i = 0; i < D / 64; ++i) {
              const int c = lane + 64 * i;
              xs[c] = a.att1[((size_t)(c / dh) * a.B + b) * a1row + (size_t)(1 + p - Ls) * dh + (c % dh)] * (P * explain_item1<DT>(a, id, c));
            }
          }
        }
        wave_lds_fence();
      }
      for (int tb = 0; tb < Ta; tb += 16) {
        const int t = tb + (lane >> 2);
        float s = 0.0f;
        if (valid) {               // (wave-uniform)
          const float* row = base + t * WS;
#pragma unroll 8
          for (int c = seg; c < D; c += 4) s += sv[c] * row[c];
          s += __shfl_xor(s, 1);
          s += __shfl_xor(s, 2);
        }
        if (seg == 0) pt[t * RS + col] = (valid && ids[t] >= 0) ? s : 0.0f;
      }
    }
  }
  __syncthreads();

  // ---- 4. the parts as the caller reads them
  if (a.parts) {
    for (int e = tid; e < Ta * R; e += 256) {
      const int t = e / R, col = e % R;
      if (t0 + t < a.Kc) a.parts[((size_t)b * a.Kc + t0 + t) * R + col] = pt[t * RS + col];
    }
  }
  if (!a.top_src) return;

  // ---- 5. by item: the leader's slot takes the sum of its members' parts, ascending columns, one rounding per addition.
  //         The barrier in front: step 4's copy of a slot to `parts` is another thread's than the one that overwrites it.
  //         Within the step only leaders' slots are written, and a leader's slot is read by its own thread alone.
  if (a.by == TLSAN_EXPLAIN_BY_ITEM) {
    __syncthreads();
    for (int e = tid; e < Ta * Rh; e += 256) {
      const int t = e / Rh, p = e % Rh;
      if (lead[p] != p) continue;
      float s = pt[t * RS + 3 + p];
      for (int k = p + 1; k < Rh; ++k)
        if (lead[k] == p) s = s + pt[t * RS + 3 + k];
      pt[t * RS + 3 + p] = s;
    }
    __syncthreads();
  }

  // ---- 6. the r best sources of every item: a thread per (item, source) ranks its own
  const int ns = *nsrc;
  for (int e = tid; e < Ta * Rh; e += 256) {
    const int t = e / Rh, p = e % Rh;
    const bool by_item = a.by == TLSAN_EXPLAIN_BY_ITEM;
    if (t0 + t >= a.Kc || ids[t] < 0 || !(by_item ? lead[p] == p : pid[p] >= 0)) continue;
    const float* row = pt + t * RS + 3;
    const float x = row[p];
    int rank = 0;
    for (int k = 0; k < Rh; ++k)
      if (k != p && (by_item ? lead[k] == k : pid[k] >= 0) && explain_better(row[k], k, x, p, a.order)) ++rank;
    if (rank < a.r) {
      const size_t at = ((size_t)b * a.Kc + t0 + t) * a.r + rank;
      a.top_src[at] = 3 + p;
      a.top_item[at] = pid[p];
      a.top_val[at] = x;
    }
  }
  for (int e = tid; e < Ta * a.r; e += 256) {      // the places no source takes
    const int t = e / a.r, k = e % a.r;
    if (t0 + t >= a.Kc || (ids[t] >= 0 && k < ns)) continue;
    const size_t at = ((size_t)b * a.Kc + t0 + t) * a.r + k;
    a.top_src[at] = -1;
    a.top_item[at] = -1;
    a.top_val[at] = 0.0f;
  }
}

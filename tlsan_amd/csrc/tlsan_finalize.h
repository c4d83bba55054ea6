// tlsan_finalize.h -- the dense half of the step's tail:
//   k_dk_partial      dK = long^T . dbridge  (split over the batch, f32 MFMA)
//   k_dense_finalize  fixed-order reduction of all dense-parameter gradient partials, and the step summary its last
//                     workgroup writes (dense_finalize_block: also the leading workgroups of k_finalize_presum and
//                     k_finalize_update, tlsan_finalize_rows.h)
#pragma once
#include "tlsan_update_args.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------
// dK[k][j] = sum_b long[b][k] * dbridge[b][j]  (gradient of tf.layers.dense's kernel,
// model.py:347): C[M=k][N=j], K-dim = samples, f32 MFMA.
// Grid: (D/64)^2 output quadrants of 64x64 x nsplit batch splits; a workgroup is 8 wavefronts and
// wavefront w of split s owns the samples [(8s+w)*spw, +spw).  A wavefront computes a whole 64x64
// quadrant for its samples from two coalesced 16-B loads per MFMA k-step: lane (q, r) reads
// channels 4r..4r+3 of sample s0+q from both operands, and float t of the load feeds MFMA tile t,
// i.e. tile ta x tb covers rows 4m+ta, columns 4n+tb -- 16 independent accumulators per k-step
// and the float4 write-out is contiguous again.  The wavefronts are summed through LDS in a
// fixed order, so a launch leaves nsplit (<= DK_SPLITS_MAX) partial matrices for k_dense_finalize.
template <int D>
__global__ __launch_bounds__(DK_WAVES * 64) void k_dk_partial(const float* __restrict__ gLong,
                                                              const float* __restrict__ gDB, int B, int spw,
                                                              float* __restrict__ Kp) {
  constexpr int NQ = D / 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [DK_WAVES wavefronts][64][64]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, r = lane & 15;
  const int quad = blockIdx.x % (NQ * NQ), split = blockIdx.x / (NQ * NQ);
  const int M0 = (quad / NQ) * 64, N0 = (quad % NQ) * 64;
  const int s_begin = (split * DK_WAVES + wave) * spw, s_end = min(s_begin + spw, B);
  f32x4 acc[4][4];
#pragma unroll
  for (int ta = 0; ta < 4; ++ta)
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = (f32x4)(0.0f);
  for (int s0 = s_begin; s0 < s_end; s0 += 16) {
    f32x4 va[4], vb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // k-step j: samples s0 + 4j + q (clamped address, zeroed past the end)
      const int sm = s0 + 4 * j + q;
      const int sc = sm < s_end ? sm : s_begin;
      va[j] = *(const f32x4*)(gLong + (size_t)sc * D + M0 + 4 * r);
      vb[j] = *(const f32x4*)(gDB + (size_t)sc * D + N0 + 4 * r);
      if (sm >= s_end) va[j] = (f32x4)(0.0f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int ta = 0; ta < 4; ++ta)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = TLSAN_MFMA(va[j][ta], vb[j][tb], acc[ta][tb]);
  }
  // acc[ta][tb][i] = C[M0 + 4 (4q + i) + ta][N0 + 4 r + tb]
  float* W = smem + wave * 4096;
#pragma unroll
  for (int ta = 0; ta < 4; ++ta)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) v[tb] = acc[ta][tb][i];
      *(f32x4*)(W + (16 * q + 4 * i + ta) * 64 + 4 * r) = v;
    }
  __syncthreads();
  float* out = Kp + (size_t)split * D * D;
#pragma unroll
  for (int k = 0; k < 1024 / (DK_WAVES * 64); ++k) {
    const int f = tid + DK_WAVES * 64 * k;  // float4 index inside the 64x64 quadrant
    f32x4 v = *(const f32x4*)(smem + 4 * f);
#pragma unroll
    for (int w_ = 1; w_ < DK_WAVES; ++w_) v += *(const f32x4*)(smem + w_ * 4096 + 4 * f);
    *(f32x4*)(out + (size_t)(M0 + f / 16) * D + N0 + 4 * (f % 16)) = v;
  }
}

// The step's scalars, computed once by the last workgroup of k_dense_finalize instead of by every
// workgroup of k_apply: global norm (tf18: per-use rows + (reg*W)^2 + dense; model.py:198-201),
// clip coefficient, loss with the L2 term (model.py:181-196), and the new table scale for lazy L2.
// Dedup-norm mode finishes the coefficient in k_clip_dedup (it needs the per-row sums first).
//
// Hand-over without a device-wide fence (a release fence would write back the whole L2, which
// holds the step's gradient rows): the few scalars other workgroups produced are published with
// returning device-scope atomics (pub_*; the wait for the returned value orders them before the
// ticket) and read back here with device-scope atomic loads.
__device__ __forceinline__ void pub_f32(float* p, float v) {
  const float old = atomicExch(p, v);
  asm volatile("" ::"v"(old));  // wait for the return: the exchange has been performed
}
__device__ __forceinline__ void pub_f64(double* p, double v) {
  const unsigned long long old = atomicExch((unsigned long long*)p, (unsigned long long)__double_as_longlong(v));
  asm volatile("" ::"v"(old));
}
__device__ __forceinline__ float acq_f32(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double acq_f64(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void step_summary(const FinArgs& a, int nsqd, double* shd) {
  const int tid = threadIdx.x;
  // (thread 0's scalars first: their round trip overlaps the partial sums')
  float P = 0.0f, sc0 = 0.0f, sc1 = 0.0f;
  double St0 = 0.0;
  if (tid == 0) {
    P = a.hdr->P;
    St0 = acq_f64(a.S_total);
    sc0 = acq_f32(a.scal + 0);
    sc1 = acq_f32(a.scal + 1);
  }
  double sq = 0.0;
  for (int k = tid; k < nsqd; k += 256) sq += (double)acq_f32(a.sqd + k);
  shd[tid] = sq;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) shd[tid] += shd[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double St = St0 * (double)P * (double)P;  // true tables = P * stored
    sq = shd[0] + (double)sc1 + (double)a.reg * (double)a.reg * St;
    const float norm = (float)sqrt(sq);
    const float coef = clip_coef(norm, a.clip);
    a.hdr->coef = coef;
    a.hdr->P_prev = P;
    if (a.count_step) a.hdr->nstep += 1;
    if (a.commit) a.hdr->P = P * (1.0f - a.lr * coef * a.reg);
    if (a.spec) {
      const float Pn = P * (1.0f - a.lr * coef * a.reg);
      const uint32_t ns = a.hdr->nstep + 1;
      a.hdr->P_next = Pn;
      a.hdr->spec_salt = ns;
      if (a.spec == 2) {
        // (the row workgroups beside this one read hdr->P_snap / nstep_snap; the next launch finds everything committed.
        //  A clipped step -- NaN included: NaN != 1 -- leaves its correction to the head of the next k_fwd_bwd or to k_spec_flush)
        a.hdr->P = Pn;
        a.hdr->nstep = ns;
        a.hdr->fix_arrive = 0;
        a.hdr->fix_ticket = 0;
        a.hdr->fix_pending = coef == 1.0f ? 0u : 1u;
      }
    }
    if (a.norm_mode == TLSAN_NORM_TF18 && a.out_gnorm) *a.out_gnorm = norm;
    if (a.out_loss) *a.out_loss = sc0 * a.inv_B + a.reg * (float)(0.5 * St);
    if (a.out_sq) *a.out_sq = sc1;
    a.hdr->ticket = 0;
  }
}

// The apply kernels leave per-workgroup CHANGES of the tables' sum of squares (DeltaRec, tagged by step): add the records
// of the last update to the running sum, once (StateHdr::folded).  One 256-thread workgroup, fixed order.  The records and
// their count are the last update's step-parity array and spart_n entry: this step's writers fill the other ones.
__device__ __forceinline__ void fold_delta(const DeltaRec* S_delta, int nrec, StateHdr* hdr, double* S_total, double* shd) {
  const int tid = threadIdx.x;
  const unsigned long long tag = hdr->nstep;     // (the records of the last update; this step's summary has not run yet)
  const DeltaRec* __restrict__ recs = delta_recs(S_delta, nrec, tag);
  // (a step's records are added once: a gradient-only call between two updates finds them folded)
  const int np = hdr->folded == (uint32_t)tag ? 0 : min(nrec, hdr->spart_n[tag & 1]);
  double s = 0.0;
  for (int k0 = tid; k0 < np; k0 += 256 * 8) {     // 8 records in flight (clamped addresses, masked sum), fixed order
    DeltaRec t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = recs[k0 + 256 * u < np ? k0 + 256 * u : k0];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (k0 + 256 * u < np && t[u].tag == tag) ? t[u].v : 0.0;
  }
  shd[tid] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) shd[tid] += shd[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    pub_f64(S_total, *S_total + shd[0]);
    hdr->folded = (uint32_t)tag;
  }
}

// Grid: [0, nbK) blocks reduce the D*D kernel gradient over the batch splits (one thread per
// entry); [nbK, nbK+nbS) blocks reduce the small parameters over the per-pass partial records
// with a lane per parameter (64 per block; a wavefront per quarter of the records, fixed order);
// the last block reduces S_part -> S_total.  Every sum has a fixed order -> deterministic.
template <int D, int DH>
__device__ __forceinline__ void dense_finalize_block(const FinArgs& a, int nbK, int nbS, int blk, double* shd, int* sh_last) {
  using G = Geo<D, DH>;
  constexpr int CW = G::CW, NPB = G::NPB, HPC = CW / DH;  // heads per 16-wide column block
  const int tid = threadIdx.x;
  const tlsan_dense_layout& L = a.lay;
  if (blk == nbK + nbS) {
    // the apply kernels leave per-workgroup CHANGES of the tables' sum of squares: fold the last
    // update's in (once)
    // (only the entries the last update can have written: a lazy update of a 10^7-row table leaves
    //  a few thousand, not rows / 16)
    fold_delta(a.S_delta, a.delta_nrec, a.hdr, a.S_total, shd);
    __syncthreads();  // shd is reused below
  }
  float g = 0.0f;
  bool owner = false;
  if (blk == nbK + nbS) {
  } else if (blk < nbK) {
    const int idx = blk * 256 + tid;
    if (idx < D * D) {
      // (spec == 2: the parameter travels beside the partials, no dependent trip)
      const float w_spec = a.spec == 2 ? a.spec_w[L.K + idx] : 0.0f;
      // the partials in chunks of KCH, all loads of a chunk in flight at once (clamped addresses, masked sum), fixed order
      // (64 since round 5: 256 partials in four dependent rounds instead of eight, about 2 us each; the sum's order does
      //  not depend on the chunk.  Measured and not kept, profiles/r05_cate_lists.md: 64 entries per workgroup with a
      //  wavefront per class of partials -- 256 workgroups, one round -- delays the row sums behind them by more than
      //  it gains; 256 B of padding between the partials, against channel conflicts of the 64 KB stride, is slower)
      //  (32 when there are no more partials than that -- k_dk_partial's launches at d = 256: clamped loads are still loads)
      float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f;
      auto chunks = [&](auto kch) {
        constexpr int KCH = decltype(kch)::value;
        for (int s0 = 0; s0 < a.nsplit; s0 += KCH) {
          float v[KCH];
#pragma unroll
          for (int u = 0; u < KCH; ++u)
            v[u] = a.Kp[(size_t)min(s0 + u, a.nsplit - 1) * D * D + idx];
#pragma unroll
          for (int u = 0; u < KCH; u += 4) {
            g0 += s0 + u + 0 < a.nsplit ? v[u + 0] : 0.0f;
            g1 += s0 + u + 1 < a.nsplit ? v[u + 1] : 0.0f;
            g2 += s0 + u + 2 < a.nsplit ? v[u + 2] : 0.0f;
            g3 += s0 + u + 3 < a.nsplit ? v[u + 3] : 0.0f;
          }
        }
      };
      if (a.nsplit > 32) chunks(std::integral_constant<int, TLSAN_KCH>());
      else chunks(std::integral_constant<int, 32>());
      g = (g0 + g1) + (g2 + g3);
      a.gd[L.K + idx] = g;
      if (a.spec == 2) {   // (k_spec_commit's expression with coefficient 1: lr * 1 is lr; dense_store)
        const float wn = w_spec - a.lr * g;
        a.spec_w[L.K + idx] = wn;
        a.spec_wKT[(size_t)(idx % D) * D + idx / D] = wn;
      }
      owner = true;
    }
  } else if constexpr (D > 128) {
    // d = 256: FIN_SMALL_PB = 64 parameters per workgroup, a lane per parameter: consecutive parameters are consecutive entries of a
    // record, so a wavefront's load touches two lines of ONE record; the four wavefronts take a quarter of the records
    // each, 16 loads in flight, fixed order.  (Until round 6: 16 lanes per parameter, each lane its own records -- every
    // load instruction touched 16 lines 18 KB apart: at d = 256 its 281 workgroups took 8.6 us each and held a third of the
    // row launch's slots for its first 10 us.)
    const int lane = tid & 63, wave = tid >> 6;
    const int m = (blk - nbK) * FIN_SMALL_PB + lane;
    const int n_small = L.n_dense - D * D;
    const bool valid = m < n_small;
    int n = 0, e0 = 0, e1 = 0;
    bool two = false;
    if (valid) {
      n = m < L.K ? m : m + D * D;
      // map the true parameter index to 1..HPC entries of the effective-layout record
      int e[2] = {-1, -1};
      const int wofs[4] = {L.f1_W1, L.f1_W2, L.f2_W1, L.f2_W2};
      const int bofs[4] = {L.f1_b1, L.f1_b2, L.f2_b1, L.f2_b2};
      const int pw[4] = {G::P_F1W1, G::P_F1W2, G::P_F2W1, G::P_F2W2};
      const int pb[4] = {G::P_F1B1, G::P_F1B2, G::P_F2B1, G::P_F2B2};
      for (int mm = 0; mm < 4; ++mm) {
        if (n >= wofs[mm] && n < wofs[mm] + DH * DH) {
          const int k = (n - wofs[mm]) / DH, j = (n - wofs[mm]) % DH;
          for (int h = 0; h < HPC; ++h) e[h] = pw[mm] + (h * DH + k) * CW + h * DH + j;
        }
        if (n >= bofs[mm] && n < bofs[mm] + DH) {
          const int j = n - bofs[mm];
          for (int h = 0; h < HPC; ++h) e[h] = pb[mm] + h * DH + j;
        }
      }
      if (n >= L.k0 && n < L.k0 + D) e[0] = G::P_K0 + (n - L.k0);
      if (n == L.gamma) e[0] = G::P_GAMMA;
      two = HPC > 1 && e[1] >= 0;
      e0 = e[0];
      e1 = two ? e[1] : e[0];
    }
    const int q = (a.nrec + 3) / 4, r_lo = wave * q, r_hi = min(a.nrec, r_lo + q);   // this wavefront's records
    const float w_spec = (a.spec == 2 && wave == 0 && valid) ? a.spec_w[n] : 0.0f;
    float t = 0.0f;
    if (valid) {
      // (chunks of FIN_SMALL_KCH loads in flight; of 4 when a wavefront has no more records than that -- small batches: clamped loads
      //  are still loads; the sum's order does not depend on the chunk)
      auto chunks = [&](auto kch) {
        constexpr int KCH = decltype(kch)::value;
        for (int r0 = r_lo; r0 < r_hi; r0 += KCH) {
          float v0[KCH], v1[KCH];
#pragma unroll
          for (int u = 0; u < KCH; ++u) {
            const float* p = a.partials + (size_t)(r0 + u < r_hi ? r0 + u : r0) * NPB;
            v0[u] = p[e0];
            if (HPC > 1) v1[u] = p[e1];
          }
#pragma unroll
          for (int u = 0; u < KCH; ++u)
            if (r0 + u < r_hi) t += (HPC > 1 && two) ? v0[u] + v1[u] : v0[u];
        }
      };
      if (q > 4) chunks(std::integral_constant<int, FIN_SMALL_KCH>());
      else chunks(std::integral_constant<int, 4>());
    }
    float* shf = (float*)shd;   // (256 floats of the 256 doubles)
    shf[tid] = t;
    __syncthreads();
    if (wave == 0 && valid) {
      g = (shf[lane] + shf[64 + lane]) + (shf[128 + lane] + shf[192 + lane]);
      a.gd[n] = g;
      if (a.spec == 2) a.spec_w[n] = w_spec - a.lr * g;   // (never one of K's: no transposed copy)
      owner = true;
    }
    __syncthreads();   // (shd is reused below)
  
  } else {
    // (d <= 128: 16 lanes per parameter, each lane its own records -- 77 / 23 such workgroups, never the launch's long pole;
    //  the form above costs the narrow row kernels two spilled registers)
    const int m = (blk - nbK) * 16 + (tid >> 4), rl = tid & 15;
    const int n_small = L.n_dense - D * D;
    if (m < n_small) {
      const int n = m < L.K ? m : m + D * D;
      // map the true parameter index to 1..HPC entries of the effective-layout record
      int e[2] = {-1, -1};
      const int wofs[4] = {L.f1_W1, L.f1_W2, L.f2_W1, L.f2_W2};
      const int bofs[4] = {L.f1_b1, L.f1_b2, L.f2_b1, L.f2_b2};
      const int pw[4] = {G::P_F1W1, G::P_F1W2, G::P_F2W1, G::P_F2W2};
      const int pb[4] = {G::P_F1B1, G::P_F1B2, G::P_F2B1, G::P_F2B2};
      for (int mm = 0; mm < 4; ++mm) {
        if (n >= wofs[mm] && n < wofs[mm] + DH * DH) {
          const int k = (n - wofs[mm]) / DH, j = (n - wofs[mm]) % DH;
          for (int h = 0; h < HPC; ++h) e[h] = pw[mm] + (h * DH + k) * CW + h * DH + j;
        }
        if (n >= bofs[mm] && n < bofs[mm] + DH) {
          const int j = n - bofs[mm];
          for (int h = 0; h < HPC; ++h) e[h] = pb[mm] + h * DH + j;
        }
      }
      if (n >= L.k0 && n < L.k0 + D) e[0] = G::P_K0 + (n - L.k0);
      if (n == L.gamma) e[0] = G::P_GAMMA;
      float t = 0.0f;
      const bool two = HPC > 1 && e[1] >= 0;
      const int e1 = two ? e[1] : e[0];
      const float w_spec = (a.spec == 2 && rl == 0) ? a.spec_w[n] : 0.0f;
      for (int r0 = rl; r0 < a.nrec; r0 += 16 * 8) {  // 8 records in flight per lane, fixed order
        float v0[8], v1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float* p = a.partials + (size_t)(r0 + 16 * u < a.nrec ? r0 + 16 * u : r0) * NPB;
          v0[u] = p[e[0]];
          v1[u] = p[e1];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (r0 + 16 * u < a.nrec) t += two ? v0[u] + v1[u] : v0[u];
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o);
      g = t;
      if (rl == 0) {
        a.gd[n] = g;
        if (a.spec == 2) a.spec_w[n] = w_spec - a.lr * g;
        owner = true;
      }
    }
  
  }
  shd[tid] = owner ? (double)g * (double)g : 0.0;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) shd[tid] += shd[tid + o];
    __syncthreads();
  }
  if (tid == 0 && blk < nbK + nbS) pub_f32(a.sqd + blk, (float)shd[0]);
  // (in the workgroup that folds the sum-of-squares records: it ends early; the dK entry blocks end the dense chain)
  if (blk == nbK + nbS && tid < 32) {  // loss sum and per-use square sum: 16 lanes each, fixed order
    const int which = tid >> 4, rl = tid & 15;
    float t = 0.0f;
    for (int r0 = rl; r0 < a.nrec; r0 += 16 * 8) {
      float v0[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v0[u] = a.partials[(size_t)(r0 + 16 * u < a.nrec ? r0 + 16 * u : r0) * NPB + G::P_LOSS + which];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r0 + 16 * u < a.nrec) t += v0[u];
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o);
    if (rl == 0) pub_f32(a.scal + which, t);
  }
  // ---- the last workgroup to arrive sees every other one's results and writes the step summary
  __syncthreads();
  if (tid == 0) *sh_last = atomicAdd(&a.hdr->ticket, 1) == nbK + nbS;  // nbK + nbS + 1 finalize workgroups
  __syncthreads();
  if (*sh_last) step_summary(a, nbK + nbS, shd);
}

template <int D, int DH>
__global__ __launch_bounds__(256) void k_dense_finalize(FinArgs a, int nbK, int nbS) {
  __shared__ double shd[256];
  __shared__ int sh_last;
  dense_finalize_block<D, DH>(a, nbK, nbS, blockIdx.x, shd, &sh_last);
}


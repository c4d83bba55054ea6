// tlsan_topk.h -- the K best items over all items for each row of u_t (a recommendation list), selected inside
// the scoring kernel: the [B, I] score matrix (the reference's eval_logits, model.py:140) is never materialised.
//
// Order: tf.nn.top_k's -- higher score first, equal scores -> lower GLOBAL item id first; +0.0 == -0.0; a NaN
// score ranks after every other score.  Both are folded into one 64-bit key (larger = earlier):
//   hi = order-preserving image of the score (zero canonicalised, NaN -> 1, below -inf), lo = ~global id.
// Key 0 is "no item" (id -1, score -inf in the output).
//
// Selection: a workgroup owns 16 users x an item slice (the tiling of k_eval_rank / k_eval_rank_dense, whose 16x16
// tiles it computes with the same MFMA chains on the same operands -- the accumulators are bit-identical to the rank
// path's).
// Per user the LDS holds the best KP keys so far (sorted) and an append buffer of BUF keys; a score that does not
// beat the user's K-th best key so far is rejected with one compare, a survivor is appended.  When a buffer
// overflows, the workgroup sorts the buffers (bitonic), merges them into the kept lists and raises the thresholds.
// The slice's list goes to [B, nslices, K]; k_topk_merge folds the nslices lists of a row into its top K.
#pragma once
#include "tlsan_eval.h"

#define TOPK_MAX 256

struct TopkArgs {
  EvalArgs e;                 // scoring: p, u_t, B, I, di, dc, all_emb (dense form) or NULL, id_mul, id_add
  int32_t K;
  const int32_t* excl_off;    // [B + 1] row offsets into excl_ids, or NULL (no exclusion)
  const int32_t* excl_ids;    // global item ids, ascending within a row
  int32_t* ids;               // [B, gridDim.y, K]
  float* scores;              // [B, gridDim.y, K]
};

typedef unsigned long long topk_key_t;

__device__ __forceinline__ topk_key_t topk_key(float s, int gid) {
  uint32_t h;
  if (s != s) {
    h = 1u;
  } else {
    const uint32_t u = __float_as_uint(s == 0.0f ? 0.0f : s);
    h = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((topk_key_t)h << 32) | (uint32_t)~(uint32_t)gid;
}

__device__ __forceinline__ int topk_key_id(topk_key_t k) { return k ? (int)~(uint32_t)k : -1; }

__device__ __forceinline__ float topk_key_score(topk_key_t k) {
  const uint32_t h = (uint32_t)(k >> 32);
  if (k == 0) return -__builtin_inff();
  if (h == 1u) return __builtin_nanf("");
  return __uint_as_float((h & 0x80000000u) ? (h & 0x7fffffffu) : ~h);
}

template <int KP, int BUF>
struct TopkSmem {
  topk_key_t kept[16][KP];   // best KP keys so far per user, descending
  topk_key_t buf[16][BUF];   // survivors since the last selection (cnt may run past BUF: overflow)
  int cnt[16];
  int ovf[3];                // overflow flags of three consecutive phases (see topk_phase_end)
};

__device__ __forceinline__ bool topk_in_list(const int32_t* ids, int lo, int hi, int g) {
  int a = lo, b = hi;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (ids[m] < g) a = m + 1;
    else b = m;
  }
  return a < hi && ids[a] == g;
}

template <int KP, int BUF>
__device__ __forceinline__ void topk_init(TopkSmem<KP, BUF>& sm) {
  for (int p = threadIdx.x; p < 16 * KP; p += 256) (&sm.kept[0][0])[p] = 0ull;
  if (threadIdx.x < 16) sm.cnt[threadIdx.x] = 0;
  if (threadIdx.x < 3) sm.ovf[threadIdx.x] = 0;
}

// Appends a survivor to user u's buffer; false when the buffer is full (the caller keeps it for the next phase).
template <int KP, int BUF>
__device__ __forceinline__ bool topk_push(TopkSmem<KP, BUF>& sm, int u, topk_key_t key) {
  const int slot = atomicAdd(&sm.cnt[u], 1);
  if (slot >= BUF) return false;
  sm.buf[u][slot] = key;
  return true;
}

// End of an append phase (all 256 threads): true when some buffer overflowed.  Phase ph sets flag ph % 3 and thread 0
// clears the flag of phase ph + 1, which nobody sets before this barrier and nobody reads any more (its last readers,
// phase ph - 2, have passed the barrier of phase ph - 1).
template <int KP, int BUF>
__device__ __forceinline__ bool topk_phase_end(TopkSmem<KP, BUF>& sm, bool overflow, int& ph) {
  if (threadIdx.x == 0) sm.ovf[ph == 2 ? 0 : ph + 1] = 0;
  if (overflow) sm.ovf[ph] = 1;
  __syncthreads();
  const bool again = sm.ovf[ph] != 0;
  ph = ph == 2 ? 0 : ph + 1;
  return again;
}

// Folds every user's buffer into its kept list (all 256 threads; entered and left behind a barrier).
template <int KP, int BUF>
__device__ void topk_reselect(TopkSmem<KP, BUF>& sm) {
  const int t = threadIdx.x;
  for (int p = t; p < 16 * BUF; p += 256) {   // slots past the fill hold nothing
    const int u = p / BUF, j = p % BUF;
    if (j >= sm.cnt[u]) sm.buf[u][j] = 0ull;
  }
  __syncthreads();
  for (int k = 2; k <= BUF; k <<= 1) {        // bitonic sort of each buffer, descending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < 8 * BUF; p += 256) {
        const int u = p / (BUF / 2), pi = p % (BUF / 2);
        const int i = 2 * pi - (pi & (j - 1)), l = i + j;
        const topk_key_t x = sm.buf[u][i], y = sm.buf[u][l];
        if ((x < y) == ((i & k) == 0)) {
          sm.buf[u][i] = y;
          sm.buf[u][l] = x;
        }
      }
      __syncthreads();
    }
  }
  // kept (descending) against the buffer's best KP reversed: the elementwise max is a bitonic sequence that holds
  // the best KP of both; one bitonic merge sorts it
  for (int p = t; p < 16 * KP; p += 256) {
    const int u = p / KP, i = p % KP;
    const topk_key_t x = sm.kept[u][i], y = sm.buf[u][KP - 1 - i];
    if (y > x) sm.kept[u][i] = y;
  }
  __syncthreads();
  for (int j = KP >> 1; j > 0; j >>= 1) {
    for (int p = t; p < 8 * KP; p += 256) {
      const int u = p / (KP / 2), pi = p % (KP / 2);
      const int i = 2 * pi - (pi & (j - 1)), l = i + j;
      const topk_key_t x = sm.kept[u][i], y = sm.kept[u][l];
      if (x < y) {
        sm.kept[u][i] = y;
        sm.kept[u][l] = x;
      }
    }
    __syncthreads();
  }
  if (t < 16) sm.cnt[t] = 0;
  __syncthreads();
}

// After the last phase (cnt stable behind its barrier): folds what is left and writes the kept lists' first K
// entries of users u0 .. u0 + 15 (rows < B) to out[(row * nl + l) * K + j].
template <int KP, int BUF>
__device__ __forceinline__ void topk_finish(TopkSmem<KP, BUF>& sm, int u0, int B, int K, int nl, int l, int32_t* ids,
                                            float* scores) {
  bool left = false;
#pragma unroll
  for (int u = 0; u < 16; ++u) left |= sm.cnt[u] != 0;
  if (left) topk_reselect(sm);
  for (int p = threadIdx.x; p < 16 * K; p += 256) {
    const int u = p / K, j = p % K;
    if (u0 + u >= B) continue;
    const topk_key_t key = sm.kept[u][j];
    const size_t o = ((size_t)(u0 + u) * nl + l) * K + j;
    ids[o] = topk_key_id(key);
    scores[o] = topk_key_score(key);
  }
}

// Offers the thread's N keys (bit c of pend: key[c] is still to be placed) to the buffers: key c belongs to user ub + c % NT,
// whose threshold is thr[c % NT].  All 256 threads, every round: a phase appends what fits; while some buffer of the
// workgroup overflowed, the buffers are folded into the kept lists, the thresholds raised and the rest offered again.
template <int N, int NT, int KP, int BUF>
__device__ __forceinline__ void topk_offer(TopkSmem<KP, BUF>& sm, const topk_key_t (&key)[N], unsigned pend, int ub,
                                           topk_key_t (&thr)[NT], int K, int& ph) {
  bool again;
  do {
    bool ovf = false;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      if (!(pend & (1u << c))) continue;
      if (key[c] <= thr[c % NT] || topk_push(sm, ub + c % NT, key[c])) pend &= ~(1u << c);
      else ovf = true;
    }
    again = topk_phase_end(sm, ovf, ph);
    if (again) {
      topk_reselect(sm);
#pragma unroll
      for (int i = 0; i < NT; ++i) thr[i] = sm.kept[ub + i][K - 1];
    }
  } while (again);
}

// The scan behind a score policy -- k_eval_topk's loop below, in the form the similar-items lists run (tlsan_similar.h:
// SimScore).  k_eval_topk itself keeps its own text: on this loop with a policy of its own (built in the kernel or
// inside the loop), and with only score_tiles4 or only topk_offer put into its text, it measured 1-2 % slower with an
// exclusion list or at K > 64 (profiles/eval_scan.md).  So a fix to the scan's prologue, tile loop or offer loop goes
// into both; the push, the phases, the reselection and the finish are shared functions.  (Two more copies of the loop
// exist for forms it cannot take: lists_scan, tlsan_lists.h, and shelves_scan, tlsan_shelves.h -- a fix goes into all four.)
// A workgroup of grid (ceil(B/16), slices): wavefront w of slice y scores items n0 .. n0 + 63,
// n0 = (round * slices + y) * 256 + 64 w, as 4 tiles of 16 rows x 16 items (score_tiles4: DENSE from all_emb, the chains
// of k_eval_rank_dense; else through all_emb4, k_eval_rank's), and offers the eligible scores that beat their row's
// threshold.  What a score is and which rows and items are eligible is the policy's:
//   bool row(i, u)        sets up the lane's row i (row u of u_t); false: nothing is selected for it
//   void col(acc, item)   takes in a tile: its accumulator and the local item of the lane's column
//   float score(i)        row i's score of that column
//   bool may(i, gn)       whether row i may select global item gn
// Which items the positions n = 0 .. count - 1 of the scan stand for is the item mapping's (AllItems: the table, position
// n is local item n; tlsan_scope.h: a caller's subset of it):
//   int count(a)          the number of positions
//   int local(n)          the local item of position n < count, as the mapping holds it
//   bool holds(loc)       whether that is an item of the table; if not, the column reads item 0 and is never selected
// and one constant, `loaded`: whether local() reads memory.  A round's loaded locals are read a round ahead of the tiles
// that need them and looked at (holds) only when their round comes, so neither the load nor a wait for it is on the
// critical path of the tile's table loads.  Without it (AllItems) a local is arithmetic of the round itself, and the scan
// is the one k_similar_topk has always run: no register is carried from round to round for it.
// The global id of a column is local * id_mul + id_add.
struct AllItems {
  static constexpr bool loaded = false;
  __device__ __forceinline__ int count(const EvalArgs& a) const { return a.I; }
  __device__ __forceinline__ int local(int n) const { return n; }
  __device__ __forceinline__ bool holds(int) const { return true; }
};

template <int D, int KP, int BUF, bool DENSE, class Policy, class Map>
__device__ __forceinline__ void topk_scan(TopkSmem<KP, BUF>& sm, const TopkArgs& ta, Policy& pol, const Map& map) {
  const EvalArgs& a = ta.e;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * 16;
  topk_init(sm);
  f32x4 af[D / 16];
  load_user_frag<D>(a, u0, q, r, af);
  bool uv[4];
  int xlo[4], xhi[4];
  topk_key_t thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = u0 + 4 * q + i;
    uv[i] = pol.row(i, u);
    xlo[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u] : 0;
    xhi[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u + 1] : 0;
    thr[i] = 0ull;
  }
  __syncthreads();
  const int cnt = map.count(a);
  const int step = gridDim.y * 256;
  const int nround = (cnt + step - 1) / step;
  const int w0 = (blockIdx.y * 4 + wave) * 64;
  // the locals of the lane's four columns of the round that starts at position n0 (positions past the count: the last one's)
  auto locals = [&](int n0, int (&loc)[4]) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) loc[tt] = map.local(min(n0 + 16 * tt + r, cnt - 1));
  };
  int nxt[4] = {0, 0, 0, 0};   // (loaded) the coming round's
  if (Map::loaded && w0 < cnt) locals(w0, nxt);
  int ph = 0;
  for (int rd = 0; rd < nround; ++rd) {
    const int n0 = rd * step + w0;
    topk_key_t key[16];
    unsigned pend = 0;
    if (n0 < cnt) {
      int item[4];
      bool held[4];
      f32x4 acc[4];
      if (Map::loaded) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          held[tt] = map.holds(nxt[tt]);
          item[tt] = held[tt] ? nxt[tt] : 0;
        }
        if (n0 < cnt - step) locals(n0 + step, nxt);
      } else {
        locals(n0, item);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) held[tt] = true;
      }
      score_tiles4<D, DENSE>(a, af, item, q, acc);
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const bool vn = n0 + 16 * tt + r < cnt && held[tt];
        const int gn = item[tt] * a.id_mul + a.id_add;  // global item id
        pol.col(acc[tt], item[tt]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          key[4 * tt + i] = topk_key(pol.score(i), gn);
          // (the exclusion list is searched only for scores that pass the threshold)
          if (vn && uv[i] && pol.may(i, gn) && key[4 * tt + i] > thr[i] && !topk_in_list(ta.excl_ids, xlo[i], xhi[i], gn))
            pend |= 1u << (4 * tt + i);
        }
      }
    }
    topk_offer(sm, key, pend, 4 * q, thr, ta.K, ph);
  }
  topk_finish(sm, u0, a.B, ta.K, gridDim.y, blockIdx.y, ta.ids, ta.scores);
}

// grid (ceil(B/16), slices); wavefront w of slice y scores items n0 .. n0 + 63, n0 = (round * slices + y) * 256 + 64 w,
// as 4 tiles of 16 users x 16 items: DENSE -- from all_emb, the chains of k_eval_rank_dense; else through all_emb4,
// score_tile's chains (k_eval_rank).  The text of topk_scan with the score written in (see there why it is kept).
template <int D, int KP, int BUF, bool DENSE>
__global__ __launch_bounds__(256, 2) void k_eval_topk(TopkArgs ta) {
  // (score = (acc * P) + bias in two roundings, as k_eval_label forms the label's score: contracted into one FMA it
  //  differs in the last bit whenever P != 1)
#pragma clang fp contract(off)
  __shared__ TopkSmem<KP, BUF> sm;
  const EvalArgs& a = ta.e;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * 16;
  topk_init(sm);
  f32x4 af[D / 16];
  load_user_frag<D>(a, u0, q, r, af);
  const float P = a.p.scale ? *a.p.scale : 1.0f;
  bool uv[4];
  int xlo[4], xhi[4];
  topk_key_t thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = u0 + 4 * q + i;
    uv[i] = u < a.B;
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
        const float bias = a.p.item_b[(size_t)item[tt] * a.p.ld_itemb];
        const f32x4 sc = acc[tt] * P;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = sc[i] + bias;
          key[4 * tt + i] = topk_key(s, gn);
          // (the exclusion list is searched only for scores that pass the threshold)
          if (vn && uv[i] && key[4 * tt + i] > thr[i] && !topk_in_list(ta.excl_ids, xlo[i], xhi[i], gn))
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

// [B, nl, K] lists (each sorted, the lists' items disjoint) -> [B, K].  16 rows per workgroup, 16 threads per row;
// a round offers 64 entries of every row.
template <int KP, int BUF>
__global__ __launch_bounds__(256) void k_topk_merge(const int32_t* cid, const float* csc, int B, int nl, int K,
                                                    int32_t* ids, float* scores) {
  __shared__ TopkSmem<KP, BUF> sm;
  const int u = threadIdx.x >> 4, c0 = threadIdx.x & 15;
  const int u0 = blockIdx.x * 16, row = u0 + u;
  const bool rv = row < B;
  topk_init(sm);
  __syncthreads();
  const int n = nl * K;
  const int nround = (n + 63) / 64;
  topk_key_t thr[1] = {0ull};
  int ph = 0;
  for (int rd = 0; rd < nround; ++rd) {
    topk_key_t key[4];
    unsigned pend = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = rd * 64 + 16 * j + c0;
      key[j] = 0ull;
      if (rv && e < n) {
        const size_t o = (size_t)row * n + e;
        const int id = cid[o];
        if (id >= 0) key[j] = topk_key(csc[o], id);
      }
      if (key[j] > thr[0]) pend |= 1u << j;
    }
    topk_offer(sm, key, pend, u, thr, K, ph);
  }
  topk_finish(sm, u0, B, K, 1, 0, ids, scores);
}

// (kept list, append buffer) per row by K: LDS 18 / 24 / 64 KB per workgroup -- at K = 256 two workgroups share a CU
#define TOPK_DISPATCH(K, F) \
  do {                        \
    if ((K) <= 16) F(16, 128);  \
    else if ((K) <= 64) F(64, 128); \
    else F(256, 256);           \
  } while (0)

// tlsan_dense_host.h -- the host steps the entry points of the dense lists share (tlsan_dense.hip: tlsan_dense_topk and its
// workspace size; tlsan_after.hip: tlsan_dense_topk_after): the size limits, the workspace carve-up and the refusals.  Host
// code only; every function is internal to the unit that includes it.
#pragma once
#include "tlsan_host.h"
#include "tlsan_dense.h"

#define DENSE_QMAX (1 << 24)   // most queries of a call
#define DENSE_NMAX (1 << 30)   // most matrix rows of a call (the scan's positions stay inside int32 with a round to spare)

struct DenseWs {
  int32_t* ids;        // [Q, nsl, K] the slices' lists (nsl > 1)
  float* scores;
  size_t bytes;
  int nsl;
};

// The slices' lists take Q * nsl * K entries.  The room asked for is a bound on that which never shrinks when Q, N or K
// grows (nsl itself falls as the query tiles fill the chip): with ut = ceil(Q / 16) tiles and n = the slices there is
// work for, Q <= 16 ut and nsl <= min(n, 2048 / ut + 1), so Q * nsl <= min(16 ut n, 16 (2048 + ut)).
static inline void carve_dense(int32_t Q, int32_t N, int32_t K, char* base, DenseWs* w) {
  const int ut = (Q + 15) / 16, n = ((N + 63) / 64 + 3) / 4;
  w->nsl = eval_slices(ut, n);
  const size_t a = (size_t)16 * ut * n, b = (size_t)16 * (2048 + ut);
  const size_t nc = (a < b ? a : b) * (size_t)K;
  w->ids = (int32_t*)base;
  w->scores = (float*)(base ? base + al(4 * nc) : nullptr);
  w->bytes = 2 * al(4 * nc);
}

static inline int dense_sizes(const char* fn, int32_t Q, int32_t N, int32_t K) {
  if (Q < 1 || Q > DENSE_QMAX) return fail(TLSAN_E_BADARG, "%s: Q must be in 1..2^24 (got %d)", fn, Q);
  if (N < 1 || N > DENSE_NMAX) return fail(TLSAN_E_BADARG, "%s: N must be in 1..2^30 (got %d)", fn, N);
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "%s: K must be in 1..%d (got %d)", fn, TOPK_MAX, K);
  return TLSAN_OK;
}

// what the dense entry points refuse (pointers, d, sizes, the id mapping, the workspace); carves the workspace
static inline int dense_check(const char* fn, const float* q, int32_t Q, int32_t d, const float* x, int32_t N, const int32_t* excl_off,
                              const int32_t* excl_ids, int32_t id_add, int32_t K, const int32_t* ids, const float* scores, void* ws,
                              size_t ws_bytes, DenseWs* w) {
  int rc;
  if (!q || !x || !ids || !scores) return fail(TLSAN_E_BADARG, "%s: q, x, ids or scores is NULL", fn);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "%s: excl_off and excl_ids go together", fn);
  if (d != 64 && d != 128 && d != 256) return fail(TLSAN_E_UNSUPPORTED, "%s: d must be 64, 128 or 256 (got %d)", fn, d);
  if ((rc = dense_sizes(fn, Q, N, K))) return rc;
  if (id_add < 0 || (long long)id_add + N > (1LL << 31))
    return fail(TLSAN_E_BADARG, "%s: global row ids id_add + n must be non-negative int32 (got id_add %d, N %d)", fn, id_add, N);
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  carve_dense(Q, N, K, (char*)ws, w);
  if (w->bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, w->bytes, ws_bytes);
  return TLSAN_OK;
}

// the kernel arguments of a checked call
static inline DenseTopkArgs dense_args(const float* q, int32_t Q, const float* x, int32_t N, const float* q_scale, const float* q_bias,
                                       const int32_t* excl_off, const int32_t* excl_ids, int32_t id_add, int32_t K, int32_t* ids,
                                       float* scores, const DenseWs& w) {
  DenseTopkArgs da;
  memset(&da, 0, sizeof(da));
  EvalArgs& e = da.t.e;
  e.u_t = q; e.B = Q; e.I = N; e.all_emb = const_cast<float*>(x); e.id_mul = 1; e.id_add = id_add;
  da.t.K = K; da.t.excl_off = excl_off; da.t.excl_ids = excl_ids;
  da.t.ids = w.nsl > 1 ? w.ids : ids;
  da.t.scores = w.nsl > 1 ? w.scores : scores;
  da.q_scale = q_scale; da.q_bias = q_bias;
  return da;
}

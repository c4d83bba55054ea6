// tlsan_api_eval.hip -- the evaluation entry points of the C ABI (include/tlsan.h): ranks of the labels among all items,
// top-K items, similar-items lists, scoped lists, diversified lists, caller-given candidates and negative sampling.  The kernels of tlsan_eval.h are compiled
// here; the top-K, similar-items, scoped, re-ranking and candidate kernels in units of their own (tlsan_topk.hip, tlsan_similar.hip, tlsan_scope.hip, tlsan_rerank.hip, tlsan_cand.hip).
#include <stdio.h>

#include "tlsan_host.h"
#include "tlsan_eval.h"
#include "tlsan_topk.h"
#include "tlsan_similar.h"
#include "tlsan_scope.h"
#include "tlsan_scope_host.h"
#include "tlsan_rerank.h"
#include "tlsan_cand.h"

extern "C" {

// the exclusion lists of the _excl entry points and their two outputs (all NULL: none)
struct ExclOut { const int32_t* off; const int32_t* ids; int32_t* ahead; int32_t* held; };

// The one place that says which counting kernel ranks a table: the one that reads the dense item matrix when the
// workspace holds one (carve: up to EVAL_DENSE_MAX bytes), else the gathering one.  k_excl_ahead follows it.
static bool eval_rank_dense(const EvalArgs& e) { return e.all_emb != nullptr; }

static void launch_all_emb(const EvalArgs& e, int D, hipStream_t hs) {
  const int nae = (e.I * (D / 4) + 255) / 256;
  dispatch_d(D, [&](auto dd) { hipLaunchKernelGGL(k_all_emb<dd.value>, dim3(nae), dim3(256), 0, hs, e); });
}

// s_label_in == NULL: the label's score is computed here (labels index THIS table); s_label_out != NULL: only that.
static int eval_ranks_impl(const tlsan_dims* d, const tlsan_params* p, const float* u_t, const int32_t* labels, int32_t B,
                           int32_t* ranks, void* ws, size_t ws_bytes, void* stream, const float* s_label_in, int id_mul,
                           int id_add, float* s_label_out, const ExclOut* xo = nullptr) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  if (!u_t || !labels || (!ranks && !s_label_out) || B < 1) return fail(TLSAN_E_BADARG, "bad eval arguments");
  if (!ws) return fail(TLSAN_E_WORKSPACE, "ws is NULL");
  Ws w;
  carve(d, s, B, 0, (char*)ws, &w);
  if (w.bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "workspace too small: need %zu have %zu", w.bytes, ws_bytes);
  hipStream_t hs = (hipStream_t)stream;
  EvalArgs e = eval_args(d, p, u_t, B, id_mul, id_add);
  e.labels = labels; e.ranks = ranks; e.all_emb = w.all_emb;
  e.s_label = s_label_out ? s_label_out : (s_label_in ? const_cast<float*>(s_label_in) : w.s_label);
  if (ranks && hipMemsetAsync(ranks, 0, sizeof(int32_t) * (size_t)B, hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "memset ranks");
  const int ut = (B + 15) / 16;
  const int chunks = eval_slices(ut, ((d->item_count + 15) / 16 + 3) / 4);   // workgroups (4 wavefronts x 16 items) along the items
  const int ngrp = eval_slices(ut, ((d->item_count + 63) / 64 + 3) / 4);     // ... (4 wavefronts x 64 items)
  if (!s_label_in) dispatch_d(s.D, [&](auto dd) { hipLaunchKernelGGL(k_eval_label<dd.value>, dim3(ut), dim3(64), 0, hs, e); });
  if (ranks && eval_rank_dense(e)) {
    launch_all_emb(e, s.D, hs);
    dispatch_d(s.D, [&](auto dd) { hipLaunchKernelGGL(k_eval_rank_dense<dd.value>, dim3(ut, ngrp), dim3(256), 0, hs, e); });
  } else if (ranks) {
    dispatch_d(s.D, [&](auto dd) { hipLaunchKernelGGL(k_eval_rank<dd.value>, dim3(ut, chunks), dim3(256), 0, hs, e); });
  }
  CHECK_LAUNCH("k_eval");
  if (xo) {   // after the count: the dense item matrix of this call is there, and s_label holds the labels' scores
    if (hipMemsetAsync(xo->ahead, 0, sizeof(int32_t) * (size_t)B, hs) != hipSuccess ||
        hipMemsetAsync(xo->held, 0, sizeof(int32_t) * (size_t)B, hs) != hipSuccess)
      return fail(TLSAN_E_LAUNCH, "memset ahead / held");
    ExclArgs xa;
    memset(&xa, 0, sizeof(xa));
    xa.e = e; xa.excl_off = xo->off; xa.excl_ids = xo->ids; xa.ahead = xo->ahead; xa.held = xo->held;
    xa.fused = eval_rank_dense(e) ? 1 : 0;
    const hipError_t err = tlsan_launch_excl_ahead(xa, s.D, hs);
    if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_excl_ahead: %s", hipGetErrorString(err));
  }
  return TLSAN_OK;
}

int tlsan_eval_ranks(const tlsan_dims* d, const tlsan_params* p, const float* u_t, const int32_t* labels, int32_t B,
                     int32_t* ranks, void* ws, size_t ws_bytes, void* stream) {
  return eval_ranks_impl(d, p, u_t, labels, B, ranks, ws, ws_bytes, stream, nullptr, 1, 0, nullptr);
}

int tlsan_eval_label_scores(const tlsan_dims* d, const tlsan_params* p, const float* u_t, const int32_t* labels, int32_t B,
                            float* scores, void* ws, size_t ws_bytes, void* stream) {
  if (!scores) return fail(TLSAN_E_BADARG, "tlsan_eval_label_scores: scores is NULL");
  return eval_ranks_impl(d, p, u_t, labels, B, nullptr, ws, ws_bytes, stream, nullptr, 1, 0, scores);
}

int tlsan_eval_counts_shard(const tlsan_dims* d, const tlsan_params* p, const float* u_t, const float* label_scores,
                            const int32_t* labels_global, int32_t B, int32_t id_mul, int32_t id_add, int32_t* counts,
                            void* ws, size_t ws_bytes, void* stream) {
  if (!label_scores || !counts || id_mul < 1 || id_add < 0) return fail(TLSAN_E_BADARG, "tlsan_eval_counts_shard: bad arguments");
  return eval_ranks_impl(d, p, u_t, labels_global, B, counts, ws, ws_bytes, stream, label_scores, id_mul, id_add, nullptr);
}

int tlsan_eval_ranks_excl(const tlsan_dims* d, const tlsan_params* p, const float* u_t, const int32_t* labels, int32_t B,
                          const int32_t* excl_off, const int32_t* excl_ids, int32_t* ranks, int32_t* ahead, int32_t* held,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!excl_off || !excl_ids || !ranks || !ahead || !held) return fail(TLSAN_E_BADARG, "tlsan_eval_ranks_excl: NULL argument");
  const ExclOut xo = {excl_off, excl_ids, ahead, held};
  return eval_ranks_impl(d, p, u_t, labels, B, ranks, ws, ws_bytes, stream, nullptr, 1, 0, nullptr, &xo);
}

int tlsan_eval_counts_shard_excl(const tlsan_dims* d, const tlsan_params* p, const float* u_t, const float* label_scores,
                                 const int32_t* labels_global, int32_t B, int32_t id_mul, int32_t id_add,
                                 const int32_t* excl_off, const int32_t* excl_ids, int32_t* counts, int32_t* ahead,
                                 int32_t* held, void* ws, size_t ws_bytes, void* stream) {
  if (!label_scores || !counts || !excl_off || !excl_ids || !ahead || !held)
    return fail(TLSAN_E_BADARG, "tlsan_eval_counts_shard_excl: NULL argument");
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "tlsan_eval_counts_shard_excl: global ids n * id_mul + id_add must be non-negative int32");
  const ExclOut xo = {excl_off, excl_ids, ahead, held};
  return eval_ranks_impl(d, p, u_t, labels_global, B, counts, ws, ws_bytes, stream, label_scores, id_mul, id_add, nullptr, &xo);
}

// ---- top-K items over all items (tlsan_topk.h) ----
struct TopkWs {
  float* all_emb;      // dense [I, D] item matrix when it fits EVAL_DENSE_MAX (as the rank path), else NULL
  int32_t* ids;        // [B, nsl, K] the slices' lists (nsl > 1)
  float* scores;
  size_t bytes;
  int nsl;
};

static void carve_topk(const tlsan_dims* d, int D, int B, int K, char* base, TopkWs* w) {
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += al(n); return p; };
  const int nsl = w->nsl = eval_slices((B + 15) / 16, ((d->item_count + 63) / 64 + 3) / 4);   // (the rank path's slicing)
  const size_t ae = sizeof(float) * (size_t)d->item_count * D;
  w->all_emb = ae <= EVAL_DENSE_MAX ? (float*)take(ae) : nullptr;
  const size_t nc = nsl > 1 ? (size_t)B * nsl * K : 0;
  w->ids = (int32_t*)take(4 * nc);
  w->scores = (float*)take(4 * nc);
  w->bytes = o;
}

size_t tlsan_topk_workspace_bytes(const tlsan_dims* d, int32_t B, int32_t K) {
  Shape s;
  if (shape_of(d, &s) != TLSAN_OK) return 0;
  if (K < 1 || K > TOPK_MAX) { fail(TLSAN_E_BADARG, "top-K: K must be in 1..%d (got %d)", TOPK_MAX, K); return 0; }
  if (B < 1) { fail(TLSAN_E_BADARG, "top-K: B must be >= 1 (got %d)", B); return 0; }
  TopkWs w;
  carve_topk(d, s.D, B, K, nullptr, &w);
  return w.bytes;
}

int tlsan_eval_topk(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                    const int32_t* excl_off, const int32_t* excl_ids, int32_t id_mul, int32_t id_add, int32_t* ids,
                    float* scores, void* ws, size_t ws_bytes, void* stream) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  if (!u_t || !ids || !scores || B < 1) return fail(TLSAN_E_BADARG, "tlsan_eval_topk: bad arguments");
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "tlsan_eval_topk: K must be in 1..%d (got %d)", TOPK_MAX, K);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "tlsan_eval_topk: excl_off and excl_ids go together");
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "tlsan_eval_topk: global ids n * id_mul + id_add must be non-negative int32");
  if (!ws) return fail(TLSAN_E_WORKSPACE, "ws is NULL");
  TopkWs w;
  carve_topk(d, s.D, B, K, (char*)ws, &w);
  if (w.bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "workspace too small: need %zu have %zu", w.bytes, ws_bytes);
  hipStream_t hs = (hipStream_t)stream;
  TopkArgs ta;
  memset(&ta, 0, sizeof(ta));
  EvalArgs& e = ta.e = eval_args(d, p, u_t, B, id_mul, id_add);
  e.all_emb = w.all_emb;
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = w.nsl > 1 ? w.ids : ids;
  ta.scores = w.nsl > 1 ? w.scores : scores;
  if (e.all_emb) {
    launch_all_emb(e, s.D, hs);
    CHECK_LAUNCH("k_all_emb");
  }
  hipError_t err = tlsan_launch_topk(ta, s.D, w.nsl, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_eval_topk: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_topk_merge(const int32_t* cand_ids, const float* cand_scores, int32_t B, int32_t n_lists, int32_t K,
                     int32_t* ids, float* scores, void* stream) {
  if (!cand_ids || !cand_scores || !ids || !scores || B < 1 || n_lists < 1)
    return fail(TLSAN_E_BADARG, "tlsan_topk_merge: bad arguments");
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "tlsan_topk_merge: K must be in 1..%d (got %d)", TOPK_MAX, K);
  if ((long long)n_lists * K >= (1LL << 30)) return fail(TLSAN_E_UNSUPPORTED, "tlsan_topk_merge: n_lists * K too large");
  const hipError_t err = tlsan_launch_topk_merge(cand_ids, cand_scores, B, n_lists, K, ids, scores, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

// ---- similar-items lists (tlsan_similar.h) ----
// (tlsan_scope_host.h: named_refusal, a refusal of shape_of / check_params with the entry point's name in front)
int tlsan_item_vectors(const tlsan_dims* d, const tlsan_params* p, const int32_t* ids, int32_t Q, int32_t id_mul,
                       int32_t id_add, float* vec, float* inv_norm, void* stream) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal("tlsan_item_vectors", rc);
  if (!ids || !vec) return fail(TLSAN_E_BADARG, "tlsan_item_vectors: NULL argument");
  if (Q < 1) return fail(TLSAN_E_BADARG, "tlsan_item_vectors: Q must be >= 1 (got %d)", Q);
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "tlsan_item_vectors: global ids n * id_mul + id_add must be non-negative int32");
  VecArgs va;
  memset(&va, 0, sizeof(va));
  va.e = eval_args(d, p, nullptr, 0, id_mul, id_add);
  va.ids = ids; va.Q = Q; va.vec = vec; va.inv = inv_norm;
  const hipError_t err = tlsan_launch_item_vectors(va, s.D, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_item_vectors: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

struct SimWs {
  TopkWs t;            // the dense item matrix (or none) and the slices' lists, as top-K's
  float* inv;          // [I] inv of the table's items
  size_t bytes;
};

static void carve_similar(const tlsan_dims* d, int D, int Q, int K, char* base, SimWs* w) {
  carve_topk(d, D, Q, K, base, &w->t);
  w->inv = base ? (float*)(base + w->t.bytes) : nullptr;
  w->bytes = w->t.bytes + al(sizeof(float) * (size_t)d->item_count);
}

size_t tlsan_similar_workspace_bytes(const tlsan_dims* d, int32_t Q, int32_t K) {
  Shape s;
  const int rc = shape_of(d, &s);
  if (rc) { named_refusal("tlsan_similar_workspace_bytes", rc); return 0; }
  if (K < 1 || K > TOPK_MAX) { fail(TLSAN_E_BADARG, "tlsan_similar_workspace_bytes: K must be in 1..%d (got %d)", TOPK_MAX, K); return 0; }
  if (Q < 1) { fail(TLSAN_E_BADARG, "tlsan_similar_workspace_bytes: Q must be >= 1 (got %d)", Q); return 0; }
  SimWs w;
  carve_similar(d, s.D, Q, K, nullptr, &w);
  return w.bytes;
}

int tlsan_similar_topk(const tlsan_dims* d, const tlsan_params* p, const float* qvec, const float* qinv, const int32_t* qids,
                       int32_t Q, int32_t K, int32_t metric, const int32_t* excl_off, const int32_t* excl_ids,
                       int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal("tlsan_similar_topk", rc);
  if (metric != SIM_DOT && metric != SIM_COSINE)
    return fail(TLSAN_E_BADARG, "tlsan_similar_topk: metric must be TLSAN_SIM_DOT or TLSAN_SIM_COSINE (got %d)", metric);
  if (!qvec || !qids || !ids || !scores || (metric == SIM_COSINE && !qinv))
    return fail(TLSAN_E_BADARG, "tlsan_similar_topk: NULL argument");
  if (Q < 1) return fail(TLSAN_E_BADARG, "tlsan_similar_topk: Q must be >= 1 (got %d)", Q);
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "tlsan_similar_topk: K must be in 1..%d (got %d)", TOPK_MAX, K);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "tlsan_similar_topk: excl_off and excl_ids go together");
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "tlsan_similar_topk: global ids n * id_mul + id_add must be non-negative int32");
  if (!ws) return fail(TLSAN_E_WORKSPACE, "tlsan_similar_topk: ws is NULL");
  SimWs w;
  carve_similar(d, s.D, Q, K, (char*)ws, &w);
  if (w.bytes > ws_bytes)
    return fail(TLSAN_E_WORKSPACE, "tlsan_similar_topk: workspace too small: need %zu have %zu", w.bytes, ws_bytes);
  hipStream_t hs = (hipStream_t)stream;
  const int nsl = w.t.nsl;
  SimArgs sa;
  memset(&sa, 0, sizeof(sa));
  TopkArgs& ta = sa.t;
  EvalArgs& e = ta.e = eval_args(d, p, qvec, Q, id_mul, id_add);
  e.all_emb = w.t.all_emb;
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = nsl > 1 ? w.t.ids : ids;
  ta.scores = nsl > 1 ? w.t.scores : scores;
  sa.qinv = qinv; sa.qids = qids; sa.inv = w.inv; sa.metric = metric;
  hipError_t err = hipSuccess;
  // the inv pass also builds the dense item matrix; dot without one needs neither
  if ((metric == SIM_COSINE || e.all_emb) && (err = tlsan_launch_sim_prep(e, s.D, w.inv, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_sim_prep: %s", hipGetErrorString(err));
  if ((err = tlsan_launch_similar_topk(sa, s.D, nsl, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_similar_topk: %s", hipGetErrorString(err));
  if (nsl > 1 && (err = tlsan_launch_topk_merge(w.t.ids, w.t.scores, Q, nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

// ---- scoped lists (tlsan_scope.h) ----
// (tlsan_scope_host.h: ScopeWs, carve_scope, scope_check -- shared with the boosted call of tlsan_boost.hip)
size_t tlsan_scope_workspace_bytes(const tlsan_dims* d, int32_t B, int32_t K, int32_t nsub) {
  static const char* fn = "tlsan_scope_workspace_bytes";
  Shape s;
  const int rc = shape_of(d, &s);
  if (rc) { named_refusal(fn, rc); return 0; }
  if (K < 1 || K > TOPK_MAX) { fail(TLSAN_E_BADARG, "%s: K must be in 1..%d (got %d)", fn, TOPK_MAX, K); return 0; }
  if (B < 1) { fail(TLSAN_E_BADARG, "%s: B must be >= 1 (got %d)", fn, B); return 0; }
  if (nsub > d->item_count) { fail(TLSAN_E_BADARG, "%s: nsub %d exceeds the table's %d items", fn, nsub, d->item_count); return 0; }
  ScopeWs w;
  carve_scope(d, B, K, nsub, nullptr, &w);
  return w.bytes;
}

int tlsan_eval_topk_scoped(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                           const int32_t* excl_off, const int32_t* excl_ids, const int32_t* sub, int32_t nsub,
                           const int32_t* row_cate, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                           size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_eval_topk_scoped";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!u_t || !ids || !scores || B < 1) return fail(TLSAN_E_BADARG, "%s: bad arguments", fn);
  ScopeWs w;
  if ((rc = scope_check(fn, d, B, K, excl_off, excl_ids, sub, nsub, id_mul, id_add, ws, ws_bytes, &w))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  ScopedTopkArgs sa;
  memset(&sa, 0, sizeof(sa));
  TopkArgs& ta = sa.t;
  ta.e = eval_args(d, p, u_t, B, id_mul, id_add);      // (all_emb stays NULL: the gather form)
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = w.nsl > 1 ? w.ids : ids;
  ta.scores = w.nsl > 1 ? w.scores : scores;
  sa.s.sub = sub; sa.s.nsub = nsub < 0 ? 0 : nsub; sa.s.row_cate = row_cate;
  hipError_t err = tlsan_launch_scoped_topk(sa, s.D, w.nsl, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_scoped_topk: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, B, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_similar_topk_scoped(const tlsan_dims* d, const tlsan_params* p, const float* qvec, const float* qinv,
                              const int32_t* qids, int32_t Q, int32_t K, int32_t metric, const int32_t* excl_off,
                              const int32_t* excl_ids, const int32_t* sub, int32_t nsub, const int32_t* row_cate,
                              int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws, size_t ws_bytes,
                              void* stream) {
  static const char* fn = "tlsan_similar_topk_scoped";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (metric != SIM_DOT && metric != SIM_COSINE)
    return fail(TLSAN_E_BADARG, "%s: metric must be TLSAN_SIM_DOT or TLSAN_SIM_COSINE (got %d)", fn, metric);
  if (!qvec || !qids || !ids || !scores || (metric == SIM_COSINE && !qinv)) return fail(TLSAN_E_BADARG, "%s: NULL argument", fn);
  if (Q < 1) return fail(TLSAN_E_BADARG, "%s: Q must be >= 1 (got %d)", fn, Q);
  ScopeWs w;
  if ((rc = scope_check(fn, d, Q, K, excl_off, excl_ids, sub, nsub, id_mul, id_add, ws, ws_bytes, &w))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  ScopedSimArgs sa;
  memset(&sa, 0, sizeof(sa));
  TopkArgs& ta = sa.m.t;
  ta.e = eval_args(d, p, qvec, Q, id_mul, id_add);     // (all_emb stays NULL: the gather form)
  ta.K = K; ta.excl_off = excl_off; ta.excl_ids = excl_ids;
  ta.ids = w.nsl > 1 ? w.ids : ids;
  ta.scores = w.nsl > 1 ? w.scores : scores;
  sa.m.qinv = qinv; sa.m.qids = qids; sa.m.inv = w.inv; sa.m.metric = metric;
  sa.s.sub = sub; sa.s.nsub = nsub < 0 ? 0 : nsub; sa.s.row_cate = row_cate;
  hipError_t err = hipSuccess;
  const int count = scope_count(d, nsub);
  if (metric == SIM_COSINE && count > 0 && (err = tlsan_launch_scope_inv(ta.e, sa.s, count, s.D, w.inv, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_scope_inv: %s", hipGetErrorString(err));
  if ((err = tlsan_launch_scoped_similar(sa, s.D, w.nsl, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_scoped_similar: %s", hipGetErrorString(err));
  if (w.nsl > 1 && (err = tlsan_launch_topk_merge(w.ids, w.scores, Q, w.nsl, K, ids, scores, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

// ---- diversified lists (tlsan_rerank.h) ----
int tlsan_rerank(const int32_t* pool_ids, const float* pool_scores, const float* vec, const float* inv, const int32_t* cate,
                 int32_t B, int32_t N, int32_t d, int32_t K, float diversity, int32_t per_category, int32_t* ids,
                 float* scores, void* stream) {
  if (N < 1 || N > RERANK_MAX) return fail(TLSAN_E_BADARG, "tlsan_rerank: N must be in 1..%d (got %d)", RERANK_MAX, N);
  if (K < 1 || K > N) return fail(TLSAN_E_BADARG, "tlsan_rerank: K must be in 1..N (got K %d, N %d)", K, N);
  if (d != 64 && d != 128 && d != 256) return fail(TLSAN_E_UNSUPPORTED, "tlsan_rerank: d must be 64, 128 or 256 (got %d)", d);
  if (!(diversity >= 0.0f && diversity <= 1.0f))   // (a NaN fails both)
    return fail(TLSAN_E_BADARG, "tlsan_rerank: diversity must be in [0, 1] (got %g)", (double)diversity);
  if (per_category < 0) return fail(TLSAN_E_BADARG, "tlsan_rerank: per_category must be >= 0 (got %d)", per_category);
  if (B < 1 || (long long)B * N >= (1LL << 31))
    return fail(TLSAN_E_BADARG, "tlsan_rerank: B must be >= 1 and B * N below 2^31 (got B %d, N %d)", B, N);
  if (!pool_ids || !pool_scores || !vec || !inv || !cate || !ids || !scores)
    return fail(TLSAN_E_BADARG, "tlsan_rerank: NULL argument");
  RerankArgs a;
  memset(&a, 0, sizeof(a));
  a.pool_ids = pool_ids; a.pool_scores = pool_scores; a.vec = vec; a.inv = inv; a.cate = cate;
  a.B = B; a.N = N; a.K = K; a.per_category = per_category; a.diversity = diversity; a.ids = ids; a.scores = scores;
  const hipError_t err = tlsan_launch_rerank(a, d, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_rerank: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

// ---- caller-given candidates (tlsan_cand.h) ----
int tlsan_score_candidates(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t C,
                           const int32_t* cand, int32_t id_mul, int32_t id_add, float* scores, void* stream) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  if (!u_t || !cand || !scores) return fail(TLSAN_E_BADARG, "tlsan_score_candidates: NULL argument");
  if (B < 1 || C < 1) return fail(TLSAN_E_BADARG, "tlsan_score_candidates: B and C must be >= 1 (got %d, %d)", B, C);
  if ((long long)B * C >= (1LL << 31)) return fail(TLSAN_E_UNSUPPORTED, "tlsan_score_candidates: B * C overflows int32");
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "tlsan_score_candidates: global ids n * id_mul + id_add must be non-negative int32");
  CandArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.e = eval_args(d, p, u_t, B, id_mul, id_add);
  ca.C = C; ca.cand = cand; ca.scores = scores;
  const hipError_t err = tlsan_launch_score_cand(ca, s.D, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_score_cand: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_candidate_ranks(const int32_t* cand, const float* scores, int32_t B, int32_t C, int32_t* ranks, void* stream) {
  if (!cand || !scores || !ranks) return fail(TLSAN_E_BADARG, "tlsan_candidate_ranks: NULL argument");
  if (B < 1 || C < 1) return fail(TLSAN_E_BADARG, "tlsan_candidate_ranks: B and C must be >= 1 (got %d, %d)", B, C);
  const hipError_t err = tlsan_launch_cand_ranks(cand, scores, B, C, ranks, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_cand_ranks: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_sample_negatives(int32_t item_count, const int32_t* labels, int32_t B, int32_t N, uint64_t seed, int64_t row0,
                           const int32_t* excl_off, const int32_t* excl_ids, int32_t* out, void* stream) {
  if (!labels || !out) return fail(TLSAN_E_BADARG, "tlsan_sample_negatives: NULL argument");
  if (item_count < 1 || B < 1) return fail(TLSAN_E_BADARG, "tlsan_sample_negatives: item_count and B must be >= 1");
  if (N < 1 || N > NEG_MAX) return fail(TLSAN_E_BADARG, "tlsan_sample_negatives: N must be in 1..%d (got %d)", NEG_MAX, N);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "tlsan_sample_negatives: excl_off and excl_ids go together");
  NegArgs na;
  memset(&na, 0, sizeof(na));
  na.item_count = item_count; na.B = B; na.N = N; na.seed = seed; na.row0 = row0;
  na.labels = labels; na.excl_off = excl_off; na.excl_ids = excl_ids; na.out = out;
  const hipError_t err = tlsan_launch_sample_neg(na, (hipStream_t)stream);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_sample_neg: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

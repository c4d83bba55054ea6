// tlsan_scope_host.h -- the host steps the entry points of the scoped lists share (tlsan_api_eval.hip: tlsan_eval_topk_scoped,
// tlsan_similar_topk_scoped; tlsan_boost.hip: tlsan_eval_topk_scoped_boost): the scoring arguments of a table, the check of
// its id mapping, the workspace carve-up and the refusals.  Host code only; every function is internal to the unit that
// includes it.
#pragma once
#include <stdio.h>

#include "tlsan_host.h"
#include "tlsan_scope.h"

// a refusal of shape_of / check_params, with the entry point's name in front of its message
static inline int named_refusal(const char* fn, int rc) {
  char m[384];
  snprintf(m, sizeof(m), "%s", tlsan_last_error());
  return fail(rc, "%s: %s", fn, m);
}

// what every scoring kernel reads: the tables, the rows of u_t and the id mapping of this table; the rest zero
static inline EvalArgs eval_args(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t id_mul, int32_t id_add) {
  EvalArgs e;
  memset(&e, 0, sizeof(e));
  e.p = norm_params(p, d); e.u_t = u_t; e.B = B; e.I = d->item_count; e.di = d->d_item; e.dc = d->d_cate;
  e.id_mul = id_mul; e.id_add = id_add;
  return e;
}

// global ids n * id_mul + id_add of the table's items must be non-negative int32 (d NULL: left to shape_of's refusal)
static inline bool eval_ids_ok(const tlsan_dims* d, int32_t id_mul, int32_t id_add) {
  return id_mul >= 1 && id_add >= 0 && (!d || (long long)(d->item_count - 1) * id_mul + id_add < (1LL << 31));
}

struct ScopeWs {
  int32_t* ids;        // [B, nsl, K] the slices' lists (nsl > 1)
  float* scores;
  float* inv;          // [I] inv of the scope's items, by local item (the cosine form)
  size_t bytes;
  int nsl;
};

// positions of a scope: nsub, or the whole table (nsub < 0)
static inline int scope_count(const tlsan_dims* d, int32_t nsub) { return nsub < 0 ? d->item_count : nsub; }

static inline void carve_scope(const tlsan_dims* d, int B, int K, int32_t nsub, char* base, ScopeWs* w) {
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += al(n); return p; };
  const int nsl = w->nsl = eval_slices((B + 15) / 16, ((scope_count(d, nsub) + 63) / 64 + 3) / 4);
  const size_t nc = nsl > 1 ? (size_t)B * nsl * K : 0;
  w->ids = (int32_t*)take(4 * nc);
  w->scores = (float*)take(4 * nc);
  w->inv = (float*)take(sizeof(float) * (size_t)d->item_count);
  w->bytes = o;
}

// what the scoped entry points refuse about (B or Q, K, the exclusion lists, the id mapping, the scope, the workspace)
static inline int scope_check(const char* fn, const tlsan_dims* d, int32_t B, int32_t K, const int32_t* excl_off,
                              const int32_t* excl_ids, const int32_t* sub, int32_t nsub, int32_t id_mul, int32_t id_add, void* ws,
                              size_t ws_bytes, ScopeWs* w) {
  if (K < 1 || K > TOPK_MAX) return fail(TLSAN_E_BADARG, "%s: K must be in 1..%d (got %d)", fn, TOPK_MAX, K);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "%s: excl_off and excl_ids go together", fn);
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "%s: global ids n * id_mul + id_add must be non-negative int32", fn);
  if (!sub != (nsub < 0))
    return fail(TLSAN_E_BADARG, "%s: sub and nsub go together (sub NULL with nsub < 0: the whole table; got nsub %d)", fn, nsub);
  if (nsub > d->item_count)
    return fail(TLSAN_E_BADARG, "%s: nsub %d exceeds the table's %d items (sub holds distinct indices)", fn, nsub, d->item_count);
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  carve_scope(d, B, K, nsub, (char*)ws, w);
  if (w->bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, w->bytes, ws_bytes);
  return TLSAN_OK;
}

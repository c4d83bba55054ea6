// Category shelves (tlsan_shelves.h): the instantiations of the scan, their launch, the merge and the two entry points of the
// C ABI (include/tlsan.h: tlsan_shelves_workspace_bytes, tlsan_eval_shelves).  The scoring arguments (eval_args), the id
// mapping's check and named_refusal are tlsan_scope_host.h's.
#include <stdio.h>

#include "tlsan_host.h"
#include "tlsan_shelves.h"
#include "tlsan_scope_host.h"

struct ShelvesWs {
  topk_key_t* seg_keys;   // [B, nseg, S, m]
  int32_t* seg_cat;       // [B, nseg, S]
  topk_key_t* big_keys;   // [B, nbs, m]
  size_t bytes;
};

// the most segments, big lists and slices a plan may hold (the scan's grid y is nseg + nbs)
#define SHELF_UNITS_MAX 32767

static void carve_shelves(int B, int S, int m, int nseg, int nbs, char* base, ShelvesWs* w) {
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += al(n); return p; };
  w->seg_keys = (topk_key_t*)take(sizeof(topk_key_t) * (size_t)B * nseg * S * m);
  w->seg_cat = (int32_t*)take(4 * (size_t)B * nseg * S);
  w->big_keys = (topk_key_t*)take(sizeof(topk_key_t) * (size_t)B * nbs * m);
  w->bytes = o + 256;     // (never 0: 0 is the refusal)
}

// what both entries refuse about the scalars (after shape_of: d is a table)
static int shelves_scalars(const char* fn, int32_t B, int32_t S, int32_t m, int32_t nseg, int32_t nbig, int32_t nbs) {
  if (B < 1 || B > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: B must be in 1..2^24 (got %d)", fn, B);
  if (S < 1 || S > SHELF_SMAX) return fail(TLSAN_E_BADARG, "%s: S must be in 1..%d (got %d)", fn, SHELF_SMAX, S);
  if (m < 1 || m > SHELF_MMAX) return fail(TLSAN_E_BADARG, "%s: m must be in 1..%d (got %d)", fn, SHELF_MMAX, m);
  if (S * m > TOPK_MAX) return fail(TLSAN_E_BADARG, "%s: S * m must be at most %d (got %d * %d)", fn, TOPK_MAX, S, m);
  if (nseg < 0 || nseg > SHELF_UNITS_MAX) return fail(TLSAN_E_BADARG, "%s: nseg must be in 0..%d (got %d)", fn, SHELF_UNITS_MAX, nseg);
  if (nbig < 0 || nbig > SHELF_UNITS_MAX) return fail(TLSAN_E_BADARG, "%s: nbig must be in 0..%d (got %d)", fn, SHELF_UNITS_MAX, nbig);
  if (nbs < nbig || nbs > SHELF_UNITS_MAX || nbs > (long long)nbig * SHELF_SLICES_MAX)
    return fail(TLSAN_E_BADARG, "%s: nbs must be in nbig..min(%d, %d * nbig) (got %d with nbig %d)", fn, SHELF_UNITS_MAX,
                SHELF_SLICES_MAX, nbs, nbig);
  return TLSAN_OK;
}

static hipError_t launch_shelves_scan(const ShelvesArgs& a, int D, hipStream_t hs) {
  const dim3 grid((a.t.e.B + 15) / 16, a.nseg + a.nbs);
  dispatch_d(D, [&](auto d) {
    if (a.t.K <= 16) hipLaunchKernelGGL((k_shelves_scan<d.value, 16, 128>), grid, dim3(256), 0, hs, a);
    else hipLaunchKernelGGL((k_shelves_scan<d.value, 64, 128>), grid, dim3(256), 0, hs, a);
  });
  return hipGetLastError();
}

extern "C" {

size_t tlsan_shelves_workspace_bytes(const tlsan_dims* d, int32_t B, int32_t S, int32_t m, int32_t nseg, int32_t nbig, int32_t nbs) {
  static const char* fn = "tlsan_shelves_workspace_bytes";
  Shape s;
  const int rc = shape_of(d, &s);
  if (rc) { named_refusal(fn, rc); return 0; }
  if (shelves_scalars(fn, B, S, m, nseg, nbig, nbs)) return 0;
  ShelvesWs w;
  carve_shelves(B, S, m, nseg, nbs, nullptr, &w);
  return w.bytes;
}

int tlsan_eval_shelves(const tlsan_dims* d, const tlsan_params* p, const float* u_t, int32_t B, int32_t S, int32_t m,
                       int32_t min_items, int32_t rank_at, const int32_t* excl_off, const int32_t* excl_ids,
                       const int32_t* list_off, const int32_t* list_items, int32_t nlists, int32_t max_list,
                       const int32_t* seg_off, const int32_t* seg_lists, int32_t nseg, int32_t nsmall, const int32_t* big_off,
                       const int32_t* big_slices, int32_t nbig, int32_t nbs, const int32_t* skip, int32_t X, int32_t id_mul,
                       int32_t id_add, int32_t* cats, int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_eval_shelves";
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!u_t || !cats || !ids || !scores) return fail(TLSAN_E_BADARG, "%s: u_t, cats, ids or scores is NULL", fn);
  if ((rc = shelves_scalars(fn, B, S, m, nseg, nbig, nbs))) return rc;
  if (min_items < 1 || min_items > m) return fail(TLSAN_E_BADARG, "%s: min_items must be in 1..m = %d (got %d)", fn, m, min_items);
  if (rank_at < 0 || rank_at >= min_items)
    return fail(TLSAN_E_BADARG, "%s: rank_at must be in 0..min_items - 1 = %d (got %d)", fn, min_items - 1, rank_at);
  if (nlists < 1 || nlists > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: nlists must be in 1..2^24 (got %d)", fn, nlists);
  if (max_list < 0) return fail(TLSAN_E_BADARG, "%s: max_list must be >= 0 (got %d)", fn, max_list);
  if (nsmall < 0 || (nseg > 0 && nsmall < 1))
    return fail(TLSAN_E_BADARG, "%s: nsmall must be >= 0, and >= 1 with segments (got %d with nseg %d)", fn, nsmall, nseg);
  if (X < 0 || X > SHELF_SKIP_MAX) return fail(TLSAN_E_BADARG, "%s: X must be in 0..%d (got %d)", fn, SHELF_SKIP_MAX, X);
  if (!skip != (X == 0)) return fail(TLSAN_E_BADARG, "%s: skip and X go together (skip NULL with X = 0; got X %d)", fn, X);
  if (!list_off || !list_items) return fail(TLSAN_E_BADARG, "%s: list_off or list_items is NULL", fn);
  if (nseg > 0 && (!seg_off || !seg_lists)) return fail(TLSAN_E_BADARG, "%s: seg_off or seg_lists is NULL with nseg %d", fn, nseg);
  if (nbig > 0 && (!big_off || !big_slices)) return fail(TLSAN_E_BADARG, "%s: big_off or big_slices is NULL with nbig %d", fn, nbig);
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "%s: excl_off and excl_ids go together", fn);
  if (!eval_ids_ok(d, id_mul, id_add))
    return fail(TLSAN_E_BADARG, "%s: global ids n * id_mul + id_add must be non-negative int32", fn);
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  ShelvesWs w;
  carve_shelves(B, S, m, nseg, nbs, (char*)ws, &w);
  if (w.bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, w.bytes, ws_bytes);
  hipStream_t hs = (hipStream_t)stream;
  ShelvesArgs a;
  memset(&a, 0, sizeof(a));
  a.t.e = eval_args(d, p, u_t, B, id_mul, id_add);
  a.t.K = m; a.t.excl_off = excl_off; a.t.excl_ids = excl_ids;
  a.list_off = list_off; a.list_items = list_items; a.nlists = nlists;
  a.S = S; a.min_items = min_items; a.rank_at = rank_at;
  a.seg_off = seg_off; a.seg_lists = seg_lists; a.big_off = big_off; a.big_slices = big_slices;
  a.nseg = nseg; a.nsmall = nsmall; a.nbig = nbig; a.nbs = nbs;
  a.skip = skip; a.X = X;
  a.seg_keys = w.seg_keys; a.seg_cat = w.seg_cat; a.big_keys = w.big_keys;
  a.cats = cats; a.ids = ids; a.scores = scores;
  hipError_t err;
  if (nseg + nbs > 0 && (err = launch_shelves_scan(a, s.D, hs)) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "k_shelves_scan: %s", hipGetErrorString(err));
  hipLaunchKernelGGL(k_shelves_merge, dim3(B), dim3(64), 0, hs, a);
  if ((err = hipGetLastError()) != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_shelves_merge: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

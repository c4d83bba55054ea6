// The bf16 shortlist index (tlsan_shortlist.h): the instantiations, their launches and the entry points of the C ABI
// (include/tlsan.h: tlsan_shortlist_build, tlsan_shortlist_workspace_bytes, tlsan_shortlist_topk, tlsan_shortlist_select)
// with their argument checks -- nothing of the other host units is needed but fail().
#include "tlsan_host.h"
#include "tlsan_shortlist.h"

static int shortlist_d(const char* fn, int32_t d) {
  if (d != 64 && d != 128 && d != 256) return fail(TLSAN_E_UNSUPPORTED, "%s: d must be 64, 128 or 256 (got %d)", fn, d);
  return TLSAN_OK;
}

static int shortlist_n(const char* fn, int32_t N) {
  if (N < SHORTLIST_NMIN || N > SHORTLIST_NMAX)
    return fail(TLSAN_E_BADARG, "%s: N must be in %d..%d (got %d)", fn, SHORTLIST_NMIN, SHORTLIST_NMAX, N);
  return TLSAN_OK;
}

static int shortlist_sizes(const char* fn, int32_t I, int32_t B) {
  if (I < 1 || I > (1 << 30)) return fail(TLSAN_E_BADARG, "%s: I must be in 1..2^30 (got %d)", fn, I);
  if (B < 1 || B > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: B must be in 1..2^24 (got %d)", fn, B);
  return TLSAN_OK;
}

// item slices of a stage-1 launch (the slicing of k_eval_topk on the 16 SHORTLIST_T rows of a workgroup)
static int shortlist_slices(int32_t I, int32_t B, int32_t d, int32_t N) {
  const int rows = 16 * SHORTLIST_T;
  return eval_slices((B + rows - 1) / rows, ((I + 63) / 64 + 3) / 4);
}
// the slices' lists [B, nsl, N], ids and scores (nothing when one slice writes the result itself; never 0 bytes, which is
// what a refusal returns)
static size_t shortlist_bytes(int32_t I, int32_t B, int32_t d, int32_t N, int* nsl_out) {
  const int nsl = shortlist_slices(I, B, d, N);
  if (nsl_out) *nsl_out = nsl;
  const size_t one = nsl > 1 ? al(4 * (size_t)B * nsl * N) : 0;
  return 2 * one + 256;
}

template <int D, int KP, int BUF, int T>
static void launch_shortlist(const ShortlistArgs& a, dim3 grid, hipStream_t hs) {
  const size_t smem = sizeof(TopkSmem<KP, BUF>) * T;
  auto k = k_shortlist_topk<D, KP, BUF, T>;
  (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(k, grid, dim3(256), smem, hs, a);
}

extern "C" {

int tlsan_shortlist_build(const tlsan_dims* dims, const tlsan_params* p, uint16_t* vec, float* wmax, void* stream) {
  static const char* fn = "tlsan_shortlist_build";
  int rc;
  if (!dims || !p || !vec || !wmax) return fail(TLSAN_E_BADARG, "%s: dims, p, vec or wmax is NULL", fn);
  if ((rc = shortlist_d(fn, dims->d))) return rc;
  if (dims->d_item < 4 || dims->d_cate < 0 || dims->d_item % 4 || dims->d_cate % 4 || dims->d_item + dims->d_cate != dims->d)
    return fail(TLSAN_E_BADARG, "%s: d_item and d_cate must be multiples of 4 that add up to d (got %d + %d, d %d)", fn,
                dims->d_item, dims->d_cate, dims->d);
  if (dims->item_count < 1 || dims->item_count > (1 << 30))
    return fail(TLSAN_E_BADARG, "%s: item_count must be in 1..2^30 (got %d)", fn, dims->item_count);
  if (!p->item_emb || (dims->d_cate > 0 && (!p->cate_emb || !p->item_cate)))
    return fail(TLSAN_E_BADARG, "%s: item_emb, cate_emb or item_cate is NULL", fn);
  if (p->table_dtype != TLSAN_TABLE_F32 && p->table_dtype != TLSAN_TABLE_BF16)
    return fail(TLSAN_E_BADARG, "%s: unknown table_dtype %d", fn, p->table_dtype);
  hipStream_t hs = (hipStream_t)stream;
  ShortlistBuildArgs ba;
  memset(&ba, 0, sizeof(ba));
  ba.e.p = norm_params(p, dims); ba.e.I = dims->item_count; ba.e.di = dims->d_item; ba.e.dc = dims->d_cate;
  ba.vec = vec; ba.wmax = (uint32_t*)wmax;
  if (hipMemsetAsync(wmax, 0, sizeof(float), hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s: memset wmax", fn);
  dispatch_d(dims->d, [&](auto dd) {
    constexpr int per = 256 / (dd.value / 8);
    hipLaunchKernelGGL(k_shortlist_build<dd.value>, dim3((dims->item_count + per - 1) / per), dim3(256), 0, hs, ba);
  });
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_shortlist_build: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

size_t tlsan_shortlist_workspace_bytes(int32_t I, int32_t B, int32_t d, int32_t N) {
  static const char* fn = "tlsan_shortlist_workspace_bytes";
  if (shortlist_d(fn, d) || shortlist_n(fn, N) || shortlist_sizes(fn, I, B)) return 0;
  int nsl;
  const size_t need = shortlist_bytes(I, B, d, N, &nsl);
  if ((long long)B * nsl * N >= (1LL << 31)) {
    fail(TLSAN_E_UNSUPPORTED, "%s: B * slices * N overflows int32", fn);
    return 0;
  }
  return need;
}

int tlsan_shortlist_topk(const uint16_t* vec, int32_t I, int32_t d, const float* u_t, int32_t B, const float* scale,
                         const float* item_b, int32_t ld_itemb, int32_t N, const int32_t* excl_off, const int32_t* excl_ids,
                         int32_t id_mul, int32_t id_add, int32_t* ids, float* approx, void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_shortlist_topk";
  int rc;
  if (!vec || !u_t || !item_b || !ids || !approx) return fail(TLSAN_E_BADARG, "%s: vec, u_t, item_b, ids or approx is NULL", fn);
  if ((rc = shortlist_d(fn, d)) || (rc = shortlist_n(fn, N)) || (rc = shortlist_sizes(fn, I, B))) return rc;
  if (!excl_off != !excl_ids) return fail(TLSAN_E_BADARG, "%s: excl_off and excl_ids go together", fn);
  if (ld_itemb < 1) return fail(TLSAN_E_BADARG, "%s: ld_itemb must be >= 1 (got %d)", fn, ld_itemb);
  if (id_mul < 1 || id_add < 0 || (long long)(I - 1) * id_mul + id_add >= (1LL << 31))
    return fail(TLSAN_E_BADARG, "%s: global ids n * id_mul + id_add must be non-negative int32", fn);
  int nsl;
  const size_t need = shortlist_bytes(I, B, d, N, &nsl);
  if ((long long)B * nsl * N >= (1LL << 31)) return fail(TLSAN_E_UNSUPPORTED, "%s: B * slices * N overflows int32", fn);
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  if (ws_bytes < need) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, need, ws_bytes);
  hipStream_t hs = (hipStream_t)stream;
  int32_t* wid = (int32_t*)ws;
  float* wsc = (float*)((char*)ws + al(4 * (size_t)B * nsl * N));
  ShortlistArgs a;
  memset(&a, 0, sizeof(a));
  a.vec = vec; a.u_t = u_t; a.scale = scale; a.item_b = item_b; a.B = B; a.I = I; a.ld_itemb = ld_itemb; a.N = N;
  a.id_mul = id_mul; a.id_add = id_add; a.excl_off = excl_off; a.excl_ids = excl_ids;
  a.ids = nsl > 1 ? wid : ids;
  a.approx = nsl > 1 ? wsc : approx;
  const int rows = 16 * SHORTLIST_T;
  const dim3 grid((B + rows - 1) / rows, nsl);
  dispatch_d(d, [&](auto dd) {
#define SHORTLIST_L(KP, BUF) launch_shortlist<dd.value, KP, BUF, SHORTLIST_T>(a, grid, hs)
    TOPK_DISPATCH(N, SHORTLIST_L);
#undef SHORTLIST_L
  });
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_shortlist_topk: %s", hipGetErrorString(err));
  if (nsl > 1) {
#define SHORTLIST_M(KP, BUF) \
  hipLaunchKernelGGL((k_topk_merge<KP, BUF>), dim3((B + 15) / 16), dim3(256), 0, hs, wid, wsc, B, nsl, N, ids, approx)
    TOPK_DISPATCH(N, SHORTLIST_M);
#undef SHORTLIST_M
    if ((err = hipGetLastError()) != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_topk_merge: %s", hipGetErrorString(err));
  }
  return TLSAN_OK;
}

int tlsan_shortlist_select(const int32_t* sl_ids, const float* sl_exact, const float* sl_approx, const float* u_t,
                           const float* scale, const float* wmax, int32_t B, int32_t d, int32_t N, int32_t K, int32_t* ids,
                           float* scores, int32_t* certified, void* stream) {
  static const char* fn = "tlsan_shortlist_select";
  int rc;
  if (!sl_ids || !sl_exact || !sl_approx || !u_t || !wmax || !ids || !scores || !certified)
    return fail(TLSAN_E_BADARG, "%s: NULL argument", fn);
  if ((rc = shortlist_d(fn, d)) || (rc = shortlist_n(fn, N))) return rc;
  if (K < 1 || K >= N) return fail(TLSAN_E_BADARG, "%s: K must be in 1..N-1 (got K %d, N %d)", fn, K, N);
  if (B < 1 || B > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: B must be in 1..2^24 (got %d)", fn, B);
  hipStream_t hs = (hipStream_t)stream;
  ShortlistSelArgs a;
  memset(&a, 0, sizeof(a));
  a.sl_ids = sl_ids; a.sl_exact = sl_exact; a.sl_approx = sl_approx; a.u_t = u_t; a.scale = scale; a.wmax = wmax;
  a.B = B; a.N = N; a.K = K; a.ids = ids; a.scores = scores; a.certified = certified;
  const dim3 grid((B + 15) / 16);
  dispatch_d(d, [&](auto dd) {
#define SHORTLIST_S(KP, BUF) hipLaunchKernelGGL((k_shortlist_select<dd.value, KP, BUF>), grid, dim3(256), 0, hs, a)
    TOPK_DISPATCH(K, SHORTLIST_S);
#undef SHORTLIST_S
  });
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_shortlist_select: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

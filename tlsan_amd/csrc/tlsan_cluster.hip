// The clustered item index (tlsan_cluster.h): the instantiations, their launches and the entry points of the C ABI
// (include/tlsan.h: tlsan_cluster_workspace_bytes, tlsan_cluster_assign, tlsan_cluster_means, tlsan_cluster_probe) with
// their argument checks -- the calls read no table, so nothing of the other host units is needed but fail().
#include "tlsan_host.h"
#include "tlsan_cluster.h"

static int cluster_d(const char* fn, int32_t d) {
  if (d != 64 && d != 128 && d != 256) return fail(TLSAN_E_UNSUPPORTED, "%s: d must be 64, 128 or 256 (got %d)", fn, d);
  return TLSAN_OK;
}

static int cluster_c(const char* fn, int32_t C) {
  if (C < 1 || C > CLUSTER_CMAX) return fail(TLSAN_E_BADARG, "%s: C must be in 1..%d (got %d)", fn, CLUSTER_CMAX, C);
  return TLSAN_OK;
}

static int cluster_ws(const char* fn, const void* ws, size_t have, size_t need) {
  if (!ws) return fail(TLSAN_E_WORKSPACE, "%s: ws is NULL", fn);
  if (have < need) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small: need %zu have %zu", fn, need, have);
  return TLSAN_OK;
}

static size_t assign_bytes(int32_t C) { return al(sizeof(float) * (size_t)C); }
static size_t probe_bytes(int32_t B, int32_t P) { return al(sizeof(float) * (size_t)B * (size_t)P); }

extern "C" {

size_t tlsan_cluster_workspace_bytes(int32_t B, int32_t C, int32_t P) {
  static const char* fn = "tlsan_cluster_workspace_bytes";
  if (cluster_c(fn, C)) return 0;
  if (B < 0 || P < 0 || P > CLUSTER_PMAX || (long long)B * P >= (1LL << 31)) {
    fail(TLSAN_E_BADARG, "%s: want B >= 0, P in 0..%d and B * P below 2^31 (got B %d, P %d)", fn, CLUSTER_PMAX, B, P);
    return 0;
  }
  const size_t a = assign_bytes(C), p = probe_bytes(B, P);
  return a > p ? a : p;
}

int tlsan_cluster_assign(const float* x, int32_t N, int32_t d, const float* cent, int32_t C, int32_t* assign, float* dist,
                         void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_cluster_assign";
  int rc;
  if (!x || !cent || !assign) return fail(TLSAN_E_BADARG, "%s: x, cent or assign is NULL", fn);
  if ((rc = cluster_d(fn, d)) || (rc = cluster_c(fn, C))) return rc;
  if (N < 1 || N > (1 << 30)) return fail(TLSAN_E_BADARG, "%s: N must be in 1..2^30 (got %d)", fn, N);
  if ((rc = cluster_ws(fn, ws, ws_bytes, assign_bytes(C)))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  AssignArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.cent = cent; a.half = (const float*)ws; a.N = N; a.C = C; a.assign = assign; a.dist = dist;
  dispatch_d(d, [&](auto dd) {
    hipLaunchKernelGGL(k_cluster_half<dd.value>, dim3((C + 255) / 256), dim3(256), 0, hs, cent, C, (float*)ws);
    hipLaunchKernelGGL(k_cluster_assign<dd.value>, dim3((N + 63) / 64), dim3(256), 0, hs, a);
  });
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_cluster_assign: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_cluster_means(const float* x, int32_t N, const int32_t* order, const int32_t* seg_off, int32_t C, int32_t d,
                        float* cent, void* stream) {
  static const char* fn = "tlsan_cluster_means";
  int rc;
  if (!x || !order || !seg_off || !cent) return fail(TLSAN_E_BADARG, "%s: x, order, seg_off or cent is NULL", fn);
  if ((rc = cluster_d(fn, d)) || (rc = cluster_c(fn, C))) return rc;
  if (N < 1 || N > (1 << 30)) return fail(TLSAN_E_BADARG, "%s: N must be in 1..2^30 (got %d)", fn, N);
  hipStream_t hs = (hipStream_t)stream;
  dispatch_d(d, [&](auto dd) {
    hipLaunchKernelGGL(k_cluster_means<dd.value>, dim3(C), dim3(dd.value), 0, hs, x, N, order, seg_off, cent);
  });
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_cluster_means: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

int tlsan_cluster_probe(const float* q, int32_t B, int32_t d, const float* cent, const float* scale, const float* bias,
                        const int32_t* list_off, int32_t C, int32_t P, int32_t* row_lists, void* ws, size_t ws_bytes,
                        void* stream) {
  static const char* fn = "tlsan_cluster_probe";
  int rc;
  if (!q || !cent || !row_lists) return fail(TLSAN_E_BADARG, "%s: q, cent or row_lists is NULL", fn);
  if ((rc = cluster_d(fn, d)) || (rc = cluster_c(fn, C))) return rc;
  if (P < 1 || P > CLUSTER_PMAX) return fail(TLSAN_E_BADARG, "%s: P must be in 1..%d (got %d)", fn, CLUSTER_PMAX, P);
  if (B < 1 || B > (1 << 24)) return fail(TLSAN_E_BADARG, "%s: B must be in 1..2^24 (got %d)", fn, B);
  if ((rc = cluster_ws(fn, ws, ws_bytes, probe_bytes(B, P)))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  ProbeArgs pa;
  memset(&pa, 0, sizeof(pa));
  EvalArgs& e = pa.t.e;
  e.u_t = q; e.B = B; e.I = C; e.all_emb = const_cast<float*>(cent); e.id_mul = 1; e.id_add = 0;
  pa.t.K = P; pa.t.ids = row_lists; pa.t.scores = (float*)ws;
  pa.scale = scale; pa.bias = bias; pa.list_off = list_off;
  const dim3 grid((B + 15) / 16, 1);
  dispatch_d(d, [&](auto dd) {
    if (P <= 16) hipLaunchKernelGGL((k_cluster_probe<dd.value, 16, 128>), grid, dim3(256), 0, hs, pa);
    else hipLaunchKernelGGL((k_cluster_probe<dd.value, 64, 128>), grid, dim3(256), 0, hs, pa);
  });
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_cluster_probe: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

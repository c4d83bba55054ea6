// Explanations (tlsan_explain.h): the instantiations of k_explain, the choice of its tile, its launch and the entry point of
// the C ABI (include/tlsan.h: tlsan_explain).  named_refusal is tlsan_scope_host.h's.
#include <stdio.h>

#include <vector>

#include "tlsan_host.h"
#include "tlsan_eval.h"
#include "tlsan_explain.h"
#include "tlsan_scope_host.h"

// The tile of a call: the smallest of 16, 32, 64 items that holds Kc, halved until the workgroup's LDS fits.  0: not even
// 16 items fit (a session too long).
static int explain_tile(int D, int Kc, int Ls, int Rh, int* RS_out, size_t* bytes_out) {
  const int RS = (3 + Rh) | 1;      // (an odd stride: a column of the parts spreads over the banks)
  int T = Kc <= 16 ? 16 : Kc <= 32 ? 32 : EXPLAIN_TMAX;
  for (; T >= 16; T >>= 1) {
    const size_t bytes = sizeof(float) * (size_t)explain_lds(D, T, RS, Ls, Rh).total;
    if (bytes <= EXPLAIN_LDS_MAX) {
      *RS_out = RS;
      *bytes_out = bytes;
      return T;
    }
  }
  return 0;
}

template <int D, int DT>
static void launch_explain_as(const ExplainArgs& a, unsigned grid, size_t smem, hipStream_t hs) {
  auto k = k_explain<D, DT>;
  static int allowed_on = -1;       // the device whose copy of this kernel may take the whole LDS (set once, not per launch)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev != allowed_on) {
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, EXPLAIN_LDS_MAX);
    allowed_on = dev;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(256), smem, hs, a);
}

static hipError_t launch_explain(const ExplainArgs& a, int D, size_t smem, hipStream_t hs) {
  const unsigned grid = (unsigned)a.B * (unsigned)((a.Kc + a.T - 1) / a.T);
  dispatch_d(D, [&](auto d) {
    if (a.p.table_dtype == TLSAN_TABLE_BF16) launch_explain_as<d.value, TLSAN_TABLE_BF16>(a, grid, smem, hs);
    else launch_explain_as<d.value, TLSAN_TABLE_F32>(a, grid, smem, hs);
  });
  return hipGetLastError();
}

extern "C" {

int tlsan_explain(const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, const float* att0, const float* att1,
                  const int32_t* items, int32_t Kc, int32_t r, int32_t by, int32_t order, float* parts, int32_t* top_src,
                  int32_t* top_item, float* top_val, void* ws, size_t ws_bytes, void* stream) {
  static const char* fn = "tlsan_explain";
  (void)ws; (void)ws_bytes;
  Shape s;
  int rc = shape_of(d, &s);
  if (rc || (rc = check_params(p))) return named_refusal(fn, rc);
  if (!b || b->B < 1 || b->Sn < 0) return fail(TLSAN_E_BADARG, "%s: bad batch (B=%d, Sn=%d)", fn, b ? b->B : -1, b ? b->Sn : -1);
  if (!b->u || !b->hist_i || !b->hist_t || !b->sl || !b->sl_new || !b->u_cate || (b->Sn > 0 && !b->hist_i_new))
    return fail(TLSAN_E_BADARG, "%s: NULL batch pointer", fn);
  if (!att0 || !att1 || !items) return fail(TLSAN_E_BADARG, "%s: att0, att1 or items is NULL", fn);
  if (Kc < 1) return fail(TLSAN_E_BADARG, "%s: Kc must be >= 1 (got %d)", fn, Kc);
  const bool top = top_src || top_item || top_val;
  if (top && !(top_src && top_item && top_val)) return fail(TLSAN_E_BADARG, "%s: top_src, top_item and top_val go together", fn);
  if (!top && !parts) return fail(TLSAN_E_BADARG, "%s: neither parts nor top_* is asked for", fn);
  if (top && (r < 1 || r > TLSAN_EXPLAIN_RMAX)) return fail(TLSAN_E_BADARG, "%s: r must be in 1..%d (got %d)", fn, TLSAN_EXPLAIN_RMAX, r);
  if (by != TLSAN_EXPLAIN_BY_POSITION && by != TLSAN_EXPLAIN_BY_ITEM) return fail(TLSAN_E_BADARG, "%s: unknown by %d", fn, by);
  if (order != TLSAN_EXPLAIN_POSITIVE && order != TLSAN_EXPLAIN_ABS) return fail(TLSAN_E_BADARG, "%s: unknown order %d", fn, order);
  const int Rh = d->Ls + b->Sn;
  if (Rh > EXPLAIN_RH_MAX) return fail(TLSAN_E_UNSUPPORTED, "%s: Ls + Sn must be at most %d (got %d): the selection is quadratic in a row's positions", fn, EXPLAIN_RH_MAX, Rh);
  if ((long long)b->B * Kc * (3 + Rh) >= (1LL << 31)) return fail(TLSAN_E_UNSUPPORTED, "%s: B * Kc * R overflows int32", fn);
  int RS = 0;
  size_t smem = 0;
  const int T = explain_tile(s.D, Kc, d->Ls, Rh, &RS, &smem);
  if (!T) return fail(TLSAN_E_UNSUPPORTED, "%s: a 16-item tile with %d parts per item does not fit the LDS (Sn=%d)", fn, 3 + Rh, b->Sn);
  hipStream_t hs = (hipStream_t)stream;
  {  // an id past the table is refused before anything is launched: the ids come to the host for that
    const size_t n = (size_t)b->B * Kc;
    std::vector<int32_t> h(n);
    if (hipMemcpyAsync(h.data(), items, 4 * n, hipMemcpyDeviceToHost, hs) != hipSuccess || hipStreamSynchronize(hs) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TLSAN_E_LAUNCH, "%s: reading items back failed (the call cannot be captured into a graph)", fn);
    }
    for (size_t k = 0; k < n; ++k)
      if (h[k] >= d->item_count)
        return fail(TLSAN_E_BADARG, "%s: items[%zu, %zu] = %d is not below item_count %d", fn, k / Kc, k % Kc, h[k], d->item_count);
  }
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  ExplainArgs a;
  memset(&a, 0, sizeof(a));
  a.p = norm_params(p, d);
  a.B = b->B; a.Sn = b->Sn; a.Ls = d->Ls; a.dh = s.DH; a.di = d->d_item; a.dc = d->d_cate; a.Kc = Kc;
  a.T = T; a.RS = RS;
  a.r = top ? r : 0; a.by = by; a.order = order;
  a.oK = L.K; a.ok0 = L.k0; a.ogamma = L.gamma;
  a.u = b->u; a.hist_i = b->hist_i; a.hist_i_new = b->hist_i_new; a.sl = b->sl; a.sl_new = b->sl_new; a.u_cate = b->u_cate;
  a.hist_t = b->hist_t;
  a.att0 = att0; a.att1 = att1; a.items = items;
  a.parts = parts; a.top_src = top_src; a.top_item = top_item; a.top_val = top_val;
  const hipError_t err = launch_explain(a, s.D, smem, hs);
  if (err != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_explain: %s", hipGetErrorString(err));
  return TLSAN_OK;
}

}  // extern "C"

// tlsan_api_shard.hip -- the generic row apply and the row-sharded step of the C ABI (include/tlsan.h): routing plans,
// gathers, the summary, the owner-side applies (dense, lazy L2, lazy optimizers), the static step's dispatcher and the launch thread of the announced
// batches' plans.  The kernels of tlsan_rows.h and tlsan_shard.h are compiled here; the index scan and k_reduce_double
// belong to tlsan_api.hip and are reached through its launchers (tlsan_host.h).
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <sched.h>
#include <thread>
#include <stdio.h>

#include "tlsan_host.h"
#include "tlsan_index_args.h"   // ScanArgs (launch_scan)
#include "tlsan_shard.h"

// counting sort of gi.n destinations by row with the generic index kernels: clear the counts, count, scan them into `off`
// (and the fill cursors), fill the rows' lists.  bsum: launch_scan's scratch for large tables, or NULL
static int counting_sort(const GIdxArgs& gi, int32_t* off, long long* bsum, const char* clear_what, hipStream_t hs) {
  if (hipMemsetAsync(gi.cnt, 0, 4 * (size_t)gi.nrows, hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s", clear_what);
  const dim3 grid((gi.n + 255) / 256), blk(256);
  if (gi.n > 0) { hipLaunchKernelGGL(k_gidx<false>, grid, blk, 0, hs, gi); CHECK_LAUNCH("k_gidx<count>"); }
  ScanArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.cnt[0] = gi.cnt; sa.off[0] = off; sa.cur[0] = gi.cur; sa.n[0] = gi.nrows;
  const int nscan = (gi.nrows + 4095) / 4096;
  sa.blk0[0] = 0; sa.blk0[1] = nscan; sa.blk0[2] = nscan;
  const int rc = launch_scan(sa, nscan, bsum, hs);
  if (rc) return rc;
  if (gi.n > 0) { hipLaunchKernelGGL(k_gidx<true>, grid, blk, 0, hs, gi); CHECK_LAUNCH("k_gidx<fill>"); }
  return TLSAN_OK;
}

int build_cate_csr(const int32_t* item_cate, int I, int C, int32_t* cnt, int32_t* off, int32_t* cur, int32_t* items,
                   hipStream_t hs) {
  GIdxArgs gi;
  gi.dest = item_cate; gi.n = I; gi.nrows = C; gi.cnt = cnt; gi.cur = cur; gi.list = items;
  if (I <= CSR_SMALL_MAXN && C <= CSR_SMALL_MAXROWS) {   // one launch (the sharded step rebuilds this every step)
    hipLaunchKernelGGL(k_csr_small, dim3(CSR_SMALL_WG), dim3(1024), 0, hs, gi, off);
    CHECK_LAUNCH("k_csr_small");
    return TLSAN_OK;
  }
  return counting_sort(gi, off, nullptr, "memset cate_cnt", hs);
}

// the front of both routing plans: the batch's keys marked in the key space, and the scan that compacts it
static int route_mark_and_scan(const RouteArgs& a, int32_t* rank, int32_t* uniq, int32_t* n_uniq, hipStream_t hs) {
  const int nkeys = a.R * a.G;
  hipLaunchKernelGGL(k_route_mark, dim3((a.n_keys + 255) / 256), dim3(256), 0, hs, a);
  CHECK_LAUNCH("k_route_mark");
  // chunk sums of the scan: `uniq` receives at most min(n_keys, nkeys) entries, so when the key space
  // is larger than the batch its tail is free during the call (8-byte aligned slice)
  const int nscan = (nkeys + 4095) / 4096;
  const long long first = ((long long)(a.n_keys < nkeys ? a.n_keys : nkeys) + 1) / 2 * 2;
  long long* bsum = ((reinterpret_cast<uintptr_t>(uniq) & 7) == 0 && first + 2LL * nscan <= nkeys)
                        ? reinterpret_cast<long long*>(uniq + first) : nullptr;
  return scan_compact_impl(a.flags, nkeys, rank, uniq, n_uniq, bsum, hs);
}

// What ShardApplyArgs and ShardLazyArgs have in common, filled once: the shard, the received rows by source (src_off ==
// NULL: the static step's n_recv / G slots each), the category table and the workspace's partial sums.
template <class Args>
static int shard_front(Args& a, const char* who, float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item,
                       int32_t reg_user, const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv,
                       const int32_t* src_off, int32_t G, float gscale, const float* step_dev, float* cate_emb, int32_t C,
                       int32_t dc, const float* g_cate, void* ws) {
  memset(&a, 0, sizeof(a));
  a.shard = shard; a.ld = ld; a.cI = cI; a.R = R; a.W = W; a.reg_item = reg_item; a.reg_user = reg_user;
  a.vals = vals ? vals : shard; a.ldv = vals ? ldv : ld; a.rows = rows; a.n_recv = n_recv; a.G = G;
  for (int s = 0; s <= G; ++s) a.src_off[s] = src_off ? src_off[s] : s * (n_recv / G);
  if (a.src_off[0] != 0 || a.src_off[G] != n_recv) return fail(TLSAN_E_BADARG, "%s: src_off must run from 0 to n_recv", who);
  a.gscale = gscale; a.step_dev = step_dev;
  a.cate_emb = cate_emb; a.C = C; a.dc = dc; a.g_cate = g_cate;
  a.part_out = (double*)ws;
  a.nb_cate = (C + AP_ROWS_PB - 1) / AP_ROWS_PB;
  return TLSAN_OK;
}

// The two launches around every stamped owner update: the slot marks (unless the gather left them), and the closing sums
// (static step, a.stamp_dev: they advance the device's stamp; cate_delta: the category workgroups wrote changes too).
static int shard_lazy_mark(ShardLazyArgs& a, bool mark, hipStream_t hs) {
  a.nb_rows = (a.n_recv + AP_ROWS_PB - 1) / AP_ROWS_PB;
  if (a.nb_rows < 1) a.nb_rows = 1;   // (workgroup 0 commits the scale)
  if (mark) {
    hipLaunchKernelGGL(k_slot_mark64, dim3((a.n_recv + 255) / 256), dim3(256), 0, hs, a);
    CHECK_LAUNCH("k_slot_mark64");
  }
  return TLSAN_OK;
}
static int shard_lazy_reduce(const ShardLazyArgs& a, bool cate_delta, double* sumsq_out, float* sumsq_f32, hipStream_t hs) {
  // (the closing sums stay a launch of their own: taken by the last workgroup to finish they cost ~2000 same-address
  //  ticket atomics, 29 us against 7 + 4)
  hipLaunchKernelGGL(k_reduce_lazy2, dim3(2), dim3(256), 0, hs, a.part_out, a.nb_rows, a.nb_cate, sumsq_out, sumsq_f32, a.stamp_dev,
                     cate_delta ? 1 : 0);
  CHECK_LAUNCH("k_reduce_lazy2");
  return TLSAN_OK;
}

// The lazy-L2 owner update of both its entry points: the update of the rows that received gradients between the two.
static int shard_apply_lazy_launch(ShardLazyArgs& a, bool mark, double* sumsq_out, float* sumsq_f32, hipStream_t hs) {
  const int rc = shard_lazy_mark(a, mark, hs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_shard_apply_lazy, dim3(a.nb_rows + a.nb_cate), dim3(256), 0, hs, a);
  CHECK_LAUNCH("k_shard_apply_lazy");
  return shard_lazy_reduce(a, false, sumsq_out, sumsq_f32, hs);
}

extern "C" {

struct RowsWs { int32_t *cnt, *off, *cur, *list; double* part; long long* bsum; size_t bytes; int nblk; };
static void carve_rows(int32_t nrows, int32_t n, char* base, RowsWs* w) {
  size_t o = 0;
  auto take = [&](size_t nb) { char* p = base ? base + o : nullptr; o += al(nb); return p; };
  w->nblk = (nrows + AP_ROWS_PB - 1) / AP_ROWS_PB;
  w->cnt = (int32_t*)take(4 * (size_t)nrows);
  w->off = (int32_t*)take(4 * (size_t)nrows);
  w->cur = (int32_t*)take(4 * (size_t)nrows);
  w->list = (int32_t*)take(4 * (size_t)(n > 0 ? n : 1));
  w->part = (double*)take(8 * (size_t)w->nblk);
  w->bsum = (long long*)take(8 * ((size_t)nrows + 4095) / 4096);
  w->bytes = o;
}

size_t tlsan_rows_apply_workspace(int32_t nrows, int32_t n) {
  if (nrows < 1 || n < 0) return 0;
  RowsWs w;
  carve_rows(nrows, n, nullptr, &w);
  return w.bytes;
}

int tlsan_rows_apply(float* W, int32_t ld, int32_t nrows, int32_t width, int32_t reg_cols, const float* grows,
                     int32_t ldg, const int32_t* dest, int32_t n, float gscale, const float* step_dev, float reg,
                     double* sumsq_out, void* ws, size_t ws_bytes, void* stream) {
  if (!W || !step_dev || nrows < 1 || n < 0 || (n > 0 && (!grows || !dest)))
    return fail(TLSAN_E_BADARG, "tlsan_rows_apply: bad pointer / size");
  if (width < 4 || width % 4 || width > 16 * 4 * ROWS_NCH || ld < width || (n > 0 && ldg < width) || reg_cols < 0 || reg_cols > width)
    return fail(TLSAN_E_UNSUPPORTED, "tlsan_rows_apply: width must be a multiple of 4 in 4..%d", 16 * 4 * ROWS_NCH);
  if (ld % 4 || ldg % 4) return fail(TLSAN_E_UNSUPPORTED, "tlsan_rows_apply: row strides must be multiples of 4 floats");
  if (!ws) return fail(TLSAN_E_WORKSPACE, "ws is NULL");
  RowsWs w;
  carve_rows(nrows, n, (char*)ws, &w);
  if (w.bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "workspace too small: need %zu have %zu", w.bytes, ws_bytes);
  hipStream_t hs = (hipStream_t)stream;
  GIdxArgs gi;
  gi.dest = dest; gi.n = n; gi.nrows = nrows; gi.cnt = w.cnt; gi.cur = w.cur; gi.list = w.list;
  const int rc = counting_sort(gi, w.off, w.bsum, "memset cnt", hs);
  if (rc) return rc;
  RowsArgs ra;
  ra.W = W; ra.ld = ld; ra.nrows = nrows; ra.width = width; ra.reg_cols = reg_cols; ra.G = grows; ra.ldg = ldg;
  ra.cnt = w.cnt; ra.off = w.off; ra.list = w.list; ra.gscale = gscale; ra.step_dev = step_dev; ra.reg = reg;
  ra.part_out = w.part;
  hipLaunchKernelGGL(k_rows_apply, dim3(w.nblk), dim3(256), 0, hs, ra);
  CHECK_LAUNCH("k_rows_apply");
  return sumsq_out ? launch_reduce_double(w.part, w.nblk, sumsq_out, hs) : TLSAN_OK;
}

int tlsan_route_plan(const int32_t* keys, int32_t n_keys, int32_t R, int32_t G, const int32_t* cate_by_key,
                     int32_t* flags, int32_t* rank, int32_t* uniq, int32_t* n_uniq, int32_t* sendbuf, int32_t cap,
                     int32_t* cate_c, int32_t cate_pad, int32_t* comp, int32_t* counts_out, void* stream) {
  if (!keys || !cate_by_key || !flags || !rank || !uniq || !n_uniq || !sendbuf || !cate_c || !comp)
    return fail(TLSAN_E_BADARG, "tlsan_route_plan: NULL pointer");
  if (n_keys < 1 || R < 1 || G < 1 || (long long)R * G >= (1LL << 31)) return fail(TLSAN_E_BADARG, "tlsan_route_plan: bad sizes");
  if (cap < 0) return fail(TLSAN_E_BADARG, "tlsan_route_plan: cap < 0");
  const int need = R < n_keys ? R : n_keys;   // rows one owner can be asked for
  hipStream_t hs = (hipStream_t)stream;
  if (cate_pad < 0) return fail(TLSAN_E_BADARG, "tlsan_route_plan: cate_pad < 0");
  RouteArgs a;
  memset(&a, 0, sizeof(a));
  a.keys = keys; a.n_keys = n_keys; a.R = R; a.G = G; a.prefix = rank; a.uniq = uniq; a.n_uniq = n_uniq;
  a.cate_by_key = cate_by_key; a.flags = flags; a.sendbuf = sendbuf; a.cap = cap;
  a.cate_c = cate_c; a.cate_pad = cate_pad; a.comp = comp; a.counts_out = counts_out;
  a.overflow_need = cap < need ? need : 0;
  int nt = n_keys > G ? n_keys : G;
  if (cate_pad > nt) nt = cate_pad;
  const int rc = route_mark_and_scan(a, rank, uniq, n_uniq, hs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_route_finish, dim3((nt + 255) / 256), dim3(256), 0, hs, a);
  CHECK_LAUNCH("k_route_finish");
  return TLSAN_OK;
}

int tlsan_shard_gather(const float* shard, int32_t ld, int32_t R, int32_t W, const int32_t* recvbuf, int32_t cap,
                       int32_t G, int32_t n_recv, float* rows_out, int32_t* recv_rows, void* stream) {
  if (!shard || !recvbuf || n_recv < 0 || (n_recv > 0 && (!rows_out || !recv_rows)) || G < 1 || R < 1 || cap < 1)
    return fail(TLSAN_E_BADARG, "tlsan_shard_gather: bad arguments");
  if (W < 4 || W % 4 || ld < W || ld % 4) return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_gather: W, ld must be multiples of 4");
  if (n_recv == 0) return TLSAN_OK;
  GatherArgs a;
  a.shard = shard; a.ld = ld; a.W = W; a.recvbuf = recvbuf; a.cap = cap; a.G = G; a.n_recv = n_recv; a.R = R;
  a.rows_out = rows_out; a.recv_rows = recv_rows;
  hipLaunchKernelGGL(k_shard_gather, dim3((n_recv + 15) / 16), dim3(256), 0, (hipStream_t)stream, a);
  CHECK_LAUNCH("k_shard_gather");
  return TLSAN_OK;
}

static void shard_opt_fill(const tlsan_shard_optimizer* o, int kind, float lr, OptCtx* oc) {
  oc->opt = kind; oc->lr = lr; oc->b1 = o->beta1; oc->b2 = o->beta2; oc->eps = o->epsilon;
  if (kind == TLSAN_OPT_ADAM) oc->alpha = adam_alpha(lr, o->beta1, o->beta2, o->step);
}

static int shard_opt_ctx(const tlsan_shard_optimizer* o, float lr, OptCtx* oc) {
  memset(oc, 0, sizeof(*oc));
  if (!o || o->kind == TLSAN_OPT_SGD) return TLSAN_OK;
  if (o->scale) return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_optimizer: lazy L2 (scale) is for SGD only");
  if (o->kind != TLSAN_OPT_ADAM && o->kind != TLSAN_OPT_RMSPROP && o->kind != TLSAN_OPT_ADADELTA)
    return fail(TLSAN_E_BADARG, "tlsan_shard_optimizer: kind %d", o->kind);
  if (!o->shard_s1 || !o->shard_s2 || !o->cate_s1 || !o->cate_s2 || !o->dense_s1 || !o->dense_s2)
    return fail(TLSAN_E_BADARG, "tlsan_shard_optimizer: NULL accumulator");
  if (o->kind == TLSAN_OPT_ADAM && o->step < 1) return fail(TLSAN_E_BADARG, "tlsan_shard_optimizer: Adam's step counts from 1");
  shard_opt_fill(o, o->kind, lr, oc);
  return TLSAN_OK;
}

int tlsan_shard_summary(const float* flat, int32_t n_dense, int32_t n_cate, int32_t G, float lr, float reg, float clip,
                        const double* S_cate, float* dense, float* dense_KT, const tlsan_dims* d,
                        float* step_dev, float* loss_out, float* gnorm_out, void* stream) {
  return tlsan_shard_summary_opt(flat, n_dense, n_cate, G, lr, reg, clip, S_cate, dense, dense_KT, d, step_dev, loss_out,
                                 gnorm_out, nullptr, stream);
}

int tlsan_shard_summary_opt(const float* flat, int32_t n_dense, int32_t n_cate, int32_t G, float lr, float reg, float clip,
                            const double* S_cate, float* dense, float* dense_KT, const tlsan_dims* d,
                            float* step_dev, float* loss_out, float* gnorm_out, const tlsan_shard_optimizer* opt,
                            void* stream) {
  if (!flat || !S_cate || !dense || !dense_KT || !d || !step_dev || !loss_out || !gnorm_out || G < 1)
    return fail(TLSAN_E_BADARG, "tlsan_shard_summary: bad arguments");
  tlsan_dense_layout L;
  int rc = tlsan_dense_layout_of(d, &L);
  if (rc) return rc;
  if (n_dense != L.n_dense) return fail(TLSAN_E_BADARG, "tlsan_shard_summary: n_dense does not match dims");
  SummaryArgs a;
  a.flat = flat; a.n_dense = n_dense; a.n_cate = n_cate; a.G = G; a.lr = lr; a.reg = reg; a.clip = clip;
  a.S_cate = S_cate; a.dense = dense; a.dense_KT = dense_KT; a.D = d->d; a.K_off = L.K; a.k0_off = L.k0;
  a.step_dev = step_dev; a.loss_out = loss_out; a.gnorm_out = gnorm_out;
  if ((rc = shard_opt_ctx(opt, lr, &a.oc))) return rc;
  a.dense_s1 = opt ? opt->dense_s1 : nullptr; a.dense_s2 = opt ? opt->dense_s2 : nullptr;
  a.P_dev = opt ? opt->scale : nullptr;
  hipLaunchKernelGGL(k_shard_summary, dim3((n_dense + 1023) / 1024), dim3(1024), 0, (hipStream_t)stream, a);
  CHECK_LAUNCH("k_shard_summary");
  return TLSAN_OK;
}

size_t tlsan_shard_apply_workspace(int32_t R, int32_t C) {
  if (R < 1 || C < 1) return 0;
  return al(8 * (size_t)((R + AP_ROWS_PB - 1) / AP_ROWS_PB + (C + AP_ROWS_PB - 1) / AP_ROWS_PB));
}

int tlsan_shard_apply(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                      const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                      int32_t G, int32_t* slots, float gscale, const float* step_dev, float reg,
                      float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                      double* sumsq_out, float* sumsq_f32, void* ws, size_t ws_bytes, void* stream) {
  return tlsan_shard_apply_opt(shard, ld, cI, R, W, reg_item, reg_user, vals, ldv, rows, n_recv, src_off, G, slots, gscale,
                               step_dev, reg, cate_emb, C, dc, g_cate, sumsq_out, sumsq_f32, nullptr, 0.0f, ws, ws_bytes, stream);
}

int tlsan_shard_apply_opt(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                          const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                          int32_t G, int32_t* slots, float gscale, const float* step_dev, float reg,
                          float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                          double* sumsq_out, float* sumsq_f32, const tlsan_shard_optimizer* opt, float lr,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!shard || !slots || !step_dev || !cate_emb || !g_cate || !sumsq_out || !src_off || n_recv < 0 ||
      (n_recv > 0 && (!vals || !rows)))
    return fail(TLSAN_E_BADARG, "tlsan_shard_apply: bad pointer / size");
  if (G < 1 || G > SHARD_GMAX) return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_apply: 1..%d ranks", SHARD_GMAX);
  if (W < 4 || W % 4 || W > 16 * 4 * SHARD_NCH || dc % 4 || dc > 16 * 4 * SHARD_NCH || ld < W || ld % 4 ||
      (n_recv > 0 && (ldv < W || ldv % 4)) || cI < 0 || cI > R || reg_item > W || reg_user > W)
    return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_apply: widths must be multiples of 4 up to %d", 16 * 4 * SHARD_NCH);
  if (!ws || ws_bytes < tlsan_shard_apply_workspace(R, C)) return fail(TLSAN_E_WORKSPACE, "tlsan_shard_apply: workspace too small");
  ShardApplyArgs a;
  int rc = shard_front(a, "tlsan_shard_apply", shard, ld, cI, R, W, reg_item, reg_user, vals, ldv, rows, n_recv, src_off, G, gscale,
                       step_dev, cate_emb, C, dc, g_cate, ws);
  if (rc) return rc;
  a.slots = slots; a.reg = reg;
  if ((rc = shard_opt_ctx(opt, lr, &a.oc))) return rc;
  if (a.oc.opt != TLSAN_OPT_SGD) {
    a.shard_s1 = opt->shard_s1; a.shard_s2 = opt->shard_s2; a.cate_s1 = opt->cate_s1; a.cate_s2 = opt->cate_s2;
    a.bias_col = reg_item;   // fused item rows: [item_emb (reg_item columns) | item_b | pad]
  }
  a.nb_rows = (R + AP_ROWS_PB - 1) / AP_ROWS_PB;
  hipStream_t hs = (hipStream_t)stream;
  if (n_recv > 0) {
    hipLaunchKernelGGL(k_slot_mark, dim3((n_recv + 255) / 256), dim3(256), 0, hs, a);
    CHECK_LAUNCH("k_slot_mark");
  }
  hipLaunchKernelGGL(k_shard_apply, dim3(a.nb_rows + a.nb_cate), dim3(256), 0, hs, a);
  CHECK_LAUNCH("k_shard_apply");
  hipLaunchKernelGGL(k_reduce_double2, dim3(2), dim3(256), 0, hs, a.part_out, a.nb_rows, a.nb_cate, sumsq_out, sumsq_f32);
  CHECK_LAUNCH("k_reduce_double2");
  return TLSAN_OK;
}

size_t tlsan_shard_apply_lazy_workspace(int32_t n_recv, int32_t C) {
  if (n_recv < 0 || C < 1) return 0;
  return al(8 * (size_t)((n_recv + AP_ROWS_PB - 1) / AP_ROWS_PB + (C + AP_ROWS_PB - 1) / AP_ROWS_PB + 1));
}

int tlsan_shard_apply_lazy(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                           const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                           int32_t G, uint64_t* slots64, uint32_t stamp, float gscale, const float* step_dev,
                           float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                           double* sumsq_out, float* sumsq_f32, float* scale, void* ws, size_t ws_bytes, void* stream) {
  if (!shard || !slots64 || !step_dev || !cate_emb || !g_cate || !sumsq_out || !src_off || !scale || n_recv < 0 ||
      (n_recv > 0 && (!vals || !rows)))
    return fail(TLSAN_E_BADARG, "tlsan_shard_apply_lazy: bad pointer / size");
  if (G < 1 || G > SHARD_GMAX) return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_apply_lazy: 1..%d ranks", SHARD_GMAX);
  if (W < 4 || W % 4 || dc % 4 || ld < W || ld % 4 || (n_recv > 0 && (ldv < W || ldv % 4)) || cI < 0 || cI > R ||
      reg_item > W || reg_user > W || stamp == 0)
    return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_apply_lazy: widths must be multiples of 4, stamp != 0");
  if (!ws || ws_bytes < tlsan_shard_apply_lazy_workspace(n_recv, C)) return fail(TLSAN_E_WORKSPACE, "tlsan_shard_apply_lazy: workspace too small");
  ShardLazyArgs a;
  const int rc = shard_front(a, "tlsan_shard_apply_lazy", shard, ld, cI, R, W, reg_item, reg_user, vals, ldv, rows, n_recv, src_off, G,
                             gscale, step_dev, cate_emb, C, dc, g_cate, ws);
  if (rc) return rc;
  a.slots64 = (unsigned long long*)slots64; a.stamp = stamp; a.P_dev = scale;
  return shard_apply_lazy_launch(a, n_recv > 0, sumsq_out, sumsq_f32, (hipStream_t)stream);
}

int tlsan_shard_cate_use(const int32_t* cate_c, int32_t n, const int32_t* u_cate, int32_t B, int32_t C, float* use, void* stream) {
  if (!use || n < 0 || B < 0 || C < 1 || (n > 0 && !cate_c) || (B > 0 && !u_cate) || (long long)n + B >= (1LL << 31))
    return fail(TLSAN_E_BADARG, "tlsan_shard_cate_use: NULL pointer / bad size");
  hipStream_t hs = (hipStream_t)stream;
  if (hipMemsetAsync(use, 0, 4 * (size_t)C, hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "tlsan_shard_cate_use: memset");
  if (n + B > 0) {
    hipLaunchKernelGGL(k_cate_use_mark, dim3((n + B + 255) / 256), dim3(256), 0, hs, cate_c, n, u_cate, B, C, use);
    CHECK_LAUNCH("k_cate_use_mark");
  }
  return TLSAN_OK;
}

size_t tlsan_shard_apply_lazy_opt_workspace(int32_t n_recv, int32_t C) { return tlsan_shard_apply_lazy_workspace(n_recv, C); }

int tlsan_shard_apply_lazy_opt(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                               const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                               int32_t G, uint64_t* slots64, uint32_t stamp, float gscale, const float* step_dev, float reg,
                               float* cate_emb, int32_t C, int32_t dc, const float* g_cate, const float* cate_use,
                               double* sumsq_out, float* sumsq_f32, const tlsan_shard_optimizer* opt, float lr,
                               void* ws, size_t ws_bytes, void* stream) {
  const char* who = "tlsan_shard_apply_lazy_opt";
  if (!shard || !slots64 || !step_dev || !cate_emb || !g_cate || !cate_use || !sumsq_out || !src_off || !opt || n_recv < 0 ||
      (n_recv > 0 && (!vals || !rows)))
    return fail(TLSAN_E_BADARG, "%s: NULL pointer / bad size", who);
  const int kind = opt->kind & ~TLSAN_OPT_LAZY;   // (the lazy flag is what this call means: accepted, not required)
  if (kind != TLSAN_OPT_ADAM && kind != TLSAN_OPT_RMSPROP && kind != TLSAN_OPT_ADADELTA)
    return fail(TLSAN_E_BADARG, "%s: opt->kind %d: ADAM, RMSPROP or ADADELTA (SGD has tlsan_shard_apply_lazy)", who, opt->kind);
  const char* missing = !opt->shard_s1 ? "shard_s1" : !opt->shard_s2 ? "shard_s2" : !opt->cate_s1 ? "cate_s1" : !opt->cate_s2 ? "cate_s2" : nullptr;
  if (missing) return fail(TLSAN_E_BADARG, "%s: opt->%s is NULL", who, missing);
  if (kind == TLSAN_OPT_ADAM && opt->step < 1) return fail(TLSAN_E_BADARG, "%s: Adam's step counts from 1", who);
  if (opt->scale)
    return fail(TLSAN_E_UNSUPPORTED, "%s: opt->scale must be NULL: the update works on the stored values (table scale P = 1)", who);
  if (G < 1 || G > SHARD_GMAX) return fail(TLSAN_E_UNSUPPORTED, "%s: 1..%d ranks (G = %d)", who, SHARD_GMAX, G);
  if (W < 4 || W % 4 || W > 16 * 4 * SHARD_NCH || dc < 4 || dc % 4 || dc > 16 * 4 * SHARD_NCH || ld < W || ld % 4 ||
      (n_recv > 0 && (ldv < W || ldv % 4)) || cI < 0 || cI > R || reg_item < 0 || reg_item >= W || reg_user < 0 || reg_user > W ||
      C < 1 || stamp == 0)
    return fail(TLSAN_E_UNSUPPORTED, "%s: widths must be multiples of 4 up to %d (W = %d, dc = %d), reg_item < W, stamp != 0", who,
                16 * 4 * SHARD_NCH, W, dc);
  if (!ws || ws_bytes < tlsan_shard_apply_lazy_opt_workspace(n_recv, C)) return fail(TLSAN_E_WORKSPACE, "%s: workspace too small", who);
  ShardLazyOptArgs x;
  memset(&x, 0, sizeof(x));
  int rc = shard_front(x.l, who, shard, ld, cI, R, W, reg_item, reg_user, vals, ldv, rows, n_recv, src_off, G, gscale, step_dev,
                       cate_emb, C, dc, g_cate, ws);
  if (rc) return rc;
  x.l.slots64 = (unsigned long long*)slots64; x.l.stamp = stamp;
  x.reg = reg; x.cate_use = cate_use;
  shard_opt_fill(opt, kind, lr, &x.oc);
  x.shard_s1 = opt->shard_s1; x.shard_s2 = opt->shard_s2; x.cate_s1 = opt->cate_s1; x.cate_s2 = opt->cate_s2;
  hipStream_t hs = (hipStream_t)stream;
  if ((rc = shard_lazy_mark(x.l, n_recv > 0, hs))) return rc;
  const dim3 grid(x.l.nb_rows + x.l.nb_cate), blk(256);
  const int wide = W > dc ? W : dc;
  if (wide <= 64) hipLaunchKernelGGL(k_shard_apply_lazy_opt<1>, grid, blk, 0, hs, x);
  else if (wide <= 128) hipLaunchKernelGGL(k_shard_apply_lazy_opt<2>, grid, blk, 0, hs, x);
  else if (wide <= 192) hipLaunchKernelGGL(k_shard_apply_lazy_opt<3>, grid, blk, 0, hs, x);
  else hipLaunchKernelGGL(k_shard_apply_lazy_opt<4>, grid, blk, 0, hs, x);
  CHECK_LAUNCH("k_shard_apply_lazy_opt");
  return shard_lazy_reduce(x.l, true, sumsq_out, sumsq_f32, hs);
}

// ---- static-shape forms of the three calls above (include/tlsan.h): fixed `cap` row slots per (source, owner) pair
static int route_plan_static_impl(const int32_t* keys, int32_t n_keys, int32_t R, int32_t G, const int32_t* cate_by_key,
                                  int32_t* flags, int32_t* rank, int32_t* uniq, int32_t* n_uniq, int32_t* sendbuf, int32_t cap,
                                  int32_t* cate_c, int32_t* comp, int32_t* counts_out, int32_t* status, int32_t* status_host, void* stream) {
  if (!keys || !cate_by_key || !flags || !rank || !uniq || !n_uniq || !sendbuf || !cate_c || !comp || !status)
    return fail(TLSAN_E_BADARG, "tlsan_route_plan_static: NULL pointer");
  if (n_keys < 1 || R < 1 || G < 1 || (long long)R * G >= (1LL << 31)) return fail(TLSAN_E_BADARG, "tlsan_route_plan_static: bad sizes");
  if (cap < 1 || (long long)cap * G >= (1LL << 31)) return fail(TLSAN_E_BADARG, "tlsan_route_plan_static: bad cap");
  hipStream_t hs = (hipStream_t)stream;
  RouteArgs a;
  memset(&a, 0, sizeof(a));
  a.keys = keys; a.n_keys = n_keys; a.R = R; a.G = G; a.prefix = rank; a.uniq = uniq; a.n_uniq = n_uniq;
  a.cate_by_key = cate_by_key; a.flags = flags; a.sendbuf = sendbuf; a.cap = cap;
  a.cate_c = cate_c; a.cate_pad = G * cap; a.comp = comp; a.counts_out = counts_out;
  const int rc = route_mark_and_scan(a, rank, uniq, n_uniq, hs);
  if (rc) return rc;
  int nt = n_keys > G * cap ? n_keys : G * cap;
  hipLaunchKernelGGL(k_route_finish_static, dim3((nt + 255) / 256), dim3(256), 0, hs, a, status, status_host);
  CHECK_LAUNCH("k_route_finish_static");
  return TLSAN_OK;
}

int tlsan_route_plan_static(const int32_t* keys, int32_t n_keys, int32_t R, int32_t G, const int32_t* cate_by_key,
                            int32_t* flags, int32_t* rank, int32_t* uniq, int32_t* n_uniq, int32_t* sendbuf, int32_t cap,
                            int32_t* cate_c, int32_t* comp, int32_t* counts_out, int32_t* status, void* stream) {
  return route_plan_static_impl(keys, n_keys, R, G, cate_by_key, flags, rank, uniq, n_uniq, sendbuf, cap, cate_c, comp, counts_out, status, nullptr, stream);
}

int tlsan_shard_gather_static(const float* shard, int32_t ld, int32_t R, int32_t W, const int32_t* recvbuf, int32_t cap,
                              int32_t G, float* rows_out, int32_t* recv_rows, uint64_t* slots64, const uint32_t* stamp,
                              void* stream) {
  if (!shard || !recvbuf || !rows_out || !recv_rows || G < 1 || R < 1 || cap < 1 || (slots64 && !stamp))
    return fail(TLSAN_E_BADARG, "tlsan_shard_gather_static: bad arguments");
  if (W < 4 || W % 4 || ld < W || ld % 4) return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_gather_static: W, ld must be multiples of 4");
  GatherStaticArgs a;
  a.shard = shard; a.ld = ld; a.W = W; a.recvbuf = recvbuf; a.cap = cap; a.G = G; a.R = R;
  a.rows_out = rows_out; a.recv_rows = recv_rows; a.slots64 = (unsigned long long*)slots64; a.stamp_dev = stamp;
  hipLaunchKernelGGL(k_shard_gather_static, dim3((G * cap + 15) / 16), dim3(256), 0, (hipStream_t)stream, a);
  CHECK_LAUNCH("k_shard_gather_static");
  return TLSAN_OK;
}

int tlsan_shard_gather_wire_bf16(const float* shard, int32_t ld, int32_t R, int32_t d_emb, int32_t tail,
                                 const int32_t* recvbuf, int32_t cap, int32_t G, void* rows_out, int32_t pitch,
                                 int32_t* recv_rows, uint64_t* slots64, const uint32_t* stamp, void* stream) {
  if (!shard || !recvbuf || !rows_out || !recv_rows || G < 1 || R < 1 || cap < 1 || (slots64 && !stamp))
    return fail(TLSAN_E_BADARG, "tlsan_shard_gather_wire_bf16: bad arguments");
  if (d_emb < 4 || d_emb % 4 || tail < 0 || ld < d_emb + tail || ld % 4 || pitch % 16 || pitch < 2 * d_emb + 4 * tail)
    return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_gather_wire_bf16: d_emb %% 4 == 0, pitch %% 16 == 0, pitch >= 2 d_emb + 4 tail");
  GatherWireArgs w;
  w.g.shard = shard; w.g.ld = ld; w.g.W = 0; w.g.recvbuf = recvbuf; w.g.cap = cap; w.g.G = G; w.g.R = R;
  w.g.rows_out = (float*)rows_out; w.g.recv_rows = recv_rows; w.g.slots64 = (unsigned long long*)slots64; w.g.stamp_dev = stamp;
  w.d_emb = d_emb; w.tail = tail; w.pitch = pitch;
  hipLaunchKernelGGL(k_shard_gather_wire_bf16, dim3((G * cap + 15) / 16), dim3(256), 0, (hipStream_t)stream, w);
  CHECK_LAUNCH("k_shard_gather_wire_bf16");
  return TLSAN_OK;
}

int tlsan_shard_apply_lazy_static(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                                  const float* vals, int32_t ldv, const int32_t* rows, int32_t cap, int32_t G,
                                  uint64_t* slots64, uint32_t* stamp, int32_t marked, float gscale, const float* step_dev,
                                  float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                                  double* sumsq_out, float* sumsq_f32, float* scale,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (!shard || !slots64 || !stamp || !step_dev || !cate_emb || !g_cate || !sumsq_out || !scale || !vals || !rows)
    return fail(TLSAN_E_BADARG, "tlsan_shard_apply_lazy_static: NULL pointer");
  if (G < 1 || G > SHARD_GMAX) return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_apply_lazy_static: 1..%d ranks", SHARD_GMAX);
  if (cap < 1 || (long long)cap * G >= (1LL << 31)) return fail(TLSAN_E_BADARG, "tlsan_shard_apply_lazy_static: bad cap");
  if (W < 4 || W % 4 || dc % 4 || ld < W || ld % 4 || ldv < W || ldv % 4 || cI < 0 || cI > R || reg_item > W || reg_user > W)
    return fail(TLSAN_E_UNSUPPORTED, "tlsan_shard_apply_lazy_static: widths must be multiples of 4");
  const int n_recv = G * cap;
  if (!ws || ws_bytes < tlsan_shard_apply_lazy_workspace(n_recv, C)) return fail(TLSAN_E_WORKSPACE, "tlsan_shard_apply_lazy_static: workspace too small");
  ShardLazyArgs a;
  const int rc = shard_front(a, "tlsan_shard_apply_lazy_static", shard, ld, cI, R, W, reg_item, reg_user, vals, ldv, rows, n_recv, nullptr,
                             G, gscale, step_dev, cate_emb, C, dc, g_cate, ws);
  if (rc) return rc;
  a.slots64 = (unsigned long long*)slots64; a.stamp_dev = stamp; a.P_dev = scale;
  return shard_apply_lazy_launch(a, !marked, sumsq_out, sumsq_f32, (hipStream_t)stream);
}

// (no scratch: one launch whose prefix re-read grows with the square of n / 4096 -- meant for tables up
//  to a few hundred thousand entries; tlsan_route_plan scans its key space with chunk sums)
int tlsan_scan_compact(const int32_t* cnt, int32_t n, int32_t* prefix, int32_t* uniq, int32_t* n_uniq, void* stream) {
  return scan_compact_impl(cnt, n, prefix, uniq, n_uniq, nullptr, (hipStream_t)stream);
}

int tlsan_shard_plan_static(const tlsan_static_plan* p) {
  if (!p || !p->dims || !p->cp || !p->cb || !p->state) return fail(TLSAN_E_BADARG, "tlsan_shard_plan_static: NULL argument");
  hipStream_t s1 = (hipStream_t)p->stream, s2 = (hipStream_t)p->stream2;
  if (p->ev_fork && hipStreamWaitEvent(s1, (hipEvent_t)p->ev_fork, 0) != hipSuccess) return fail(TLSAN_E_LAUNCH, "wait(fork)");
  // (the overflow word reaches the pinned host copy by a store of the kernel that raises it: no copy behind the plan)
  int rc = route_plan_static_impl(p->keys, p->n_keys, p->R, p->G, p->cate_by_key, p->flags, p->rank, p->uniq, p->n_uniq,
                                  p->sendbuf, p->cap, p->cate_c, p->comp, nullptr, p->status, (int32_t*)p->status_host, p->stream);
  if (rc) return rc;
  if (p->ev_planned && hipEventRecord((hipEvent_t)p->ev_planned, s1) != hipSuccess) return fail(TLSAN_E_LAUNCH, "record(planned)");
  if ((rc = tlsan_state_recategorize(p->dims, p->cp, p->state, p->stream))) return rc;
  if (p->stream2 != nullptr) {
    if (p->ev_planned && hipStreamWaitEvent(s2, (hipEvent_t)p->ev_planned, 0) != hipSuccess) return fail(TLSAN_E_LAUNCH, "wait(planned)");
    if ((rc = tlsan_batch_index(p->dims, p->cb, p->cp->item_cate, p->state, 0, p->stream2))) return rc;
    if (p->ev_done1 && hipEventRecord((hipEvent_t)p->ev_done1, s2) != hipSuccess) return fail(TLSAN_E_LAUNCH, "record(done1)");
  } else {
    if ((rc = tlsan_batch_index(p->dims, p->cb, p->cp->item_cate, p->state, 0, p->stream))) return rc;
  }
  if (p->record_done0 && p->ev_done0 && hipEventRecord((hipEvent_t)p->ev_done0, s1) != hipSuccess) return fail(TLSAN_E_LAUNCH, "record(done0)");
  return TLSAN_OK;
}

// ---- the announced batches' plans on a launch thread of the library's own ------------------------------------------
// A plan is seven launches, a copy and four event operations on streams of its own; the step beside it is six launches
// on the main stream.  Issued by one host thread they cost it ~85 us per step for 77 us of kernels (the HIP runtime, not
// Python: scripts/shard_cprof.py), so the step was bound by its host.  With TLSAN_PLAN_ASYNC (phases bit) the plans are
// handed, by value, to one worker thread per process, which waits for the pinned word and issues them while the calling
// thread goes on with the main stream.  tlsan_shard_plans_flush() returns once the worker has issued everything handed
// to it (and reports its first error): call it before waiting on a plan's events, before re-using what a plan writes
// from the calling thread, and before a stream capture.
struct PlanJob {
  tlsan_static_plan p;
  tlsan_dims dims; tlsan_params cp; tlsan_batch cb;
  volatile uint32_t* word; uint32_t after;
  int device;
};
// (never destroyed: the worker sleeps on g_pcv when the process exits, and destroying a condition variable that has a
//  waiter blocks in glibc -- every process that had used the thread would hang at exit)
static std::mutex& g_pm = *new std::mutex;
static std::condition_variable& g_pcv = *new std::condition_variable;
static std::condition_variable& g_pidle = *new std::condition_variable;
static std::deque<PlanJob>& g_pq = *new std::deque<PlanJob>;
static bool g_pbusy = false, g_pstarted = false;
static int g_prc = 0;
static char g_pmsg[512] = "";

// a polite spin on a word the GPU writes: a pause instruction per poll, the time slice handed back every 64 polls -- the
// host normally runs ahead of the GPU, and a thread spinning flat out takes a core from the rank's own launch thread
static inline void spin_pause(unsigned long polls) {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#endif
  if ((polls & 63) == 0) sched_yield();
}

// wait (on the host) for the pinned word to say that step `after` has started; false: not within 30 s
// (sequence numbers run over the full 32 bits on both sides of the ABI: "reached" is (int32)(word - after) >= 0)
static bool wait_started(volatile uint32_t* word, uint32_t after) {
  const auto t0 = std::chrono::steady_clock::now();
  unsigned long polls = 0;
  while ((int32_t)(*word - after) < 0) {
    spin_pause(++polls);
    if ((polls & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) return false;
  }
  return true;
}

static void plan_worker() {
  for (;;) {
    PlanJob j;
    bool skip = false;
    {
      std::unique_lock<std::mutex> lk(g_pm);
      g_pcv.wait(lk, [] { return !g_pq.empty(); });
      j = g_pq.front();
      g_pq.pop_front();
      g_pbusy = true;
      skip = g_prc != 0;     // (an earlier job failed: the error is latched until the caller flushes; later jobs are dropped, not issued)
    }
    int rc = TLSAN_OK;
    if (!skip && hipSetDevice(j.device) != hipSuccess) rc = fail(TLSAN_E_LAUNCH, "plan worker: hipSetDevice(%d)", j.device);
    if (!skip && !rc && j.word != nullptr && !wait_started(j.word, j.after))
      rc = fail(TLSAN_E_LAUNCH, "plan worker: step %u did not start within 30 s", j.after);
    if (!skip && !rc) {
      j.p.dims = &j.dims; j.p.cp = &j.cp; j.p.cb = &j.cb;
      rc = tlsan_shard_plan_static(&j.p);
    }
    {
      std::lock_guard<std::mutex> lk(g_pm);
      if (rc && !g_prc) { g_prc = rc; snprintf(g_pmsg, sizeof(g_pmsg), "%s", tlsan_last_error()); }   // (this thread's own message)
      g_pbusy = false;
      if (g_pq.empty()) g_pidle.notify_all();
    }
  }
}

int tlsan_shard_plans_flush(void) {
  std::unique_lock<std::mutex> lk(g_pm);
  g_pidle.wait(lk, [] { return g_pq.empty() && !g_pbusy; });
  if (g_prc) {
    const int rc = g_prc;
    g_prc = 0;
    return fail(rc, "%s", g_pmsg);
  }
  return TLSAN_OK;
}

int tlsan_shard_step_static(const tlsan_static_step* s, int32_t phases, const tlsan_static_plan* const* plans, int32_t n_plans,
                            void* stream) {
  if (!s) return fail(TLSAN_E_BADARG, "tlsan_shard_step_static: NULL argument");
  int rc;
  if (phases & TLSAN_PHASE_GATHER) {
    if (s->wire) rc = tlsan_shard_gather_wire_bf16(s->shard, s->ld, s->R, s->d_emb, s->tail, s->recvbuf, s->cap, s->G, s->rows_out,
                                                   s->pitch, s->recv_rows, s->slots64, s->stamp, stream);
    else rc = tlsan_shard_gather_static(s->shard, s->ld, s->R, s->W, s->recvbuf, s->cap, s->G, (float*)s->rows_out, s->recv_rows,
                                        s->slots64, s->stamp, stream);
    if (rc) return rc;
  }
  if (phases & TLSAN_PHASE_GRADS) {
    if ((rc = tlsan_grads(s->dims, s->cp, s->cb, &s->hp, &s->go, &s->out, s->state, s->ws, s->ws_bytes, stream))) return rc;
  }
  if (phases & TLSAN_PHASE_SUMMARY) {
    if ((rc = tlsan_shard_summary_opt(s->flat, s->n_dense, s->n_cate, s->G, s->lr, s->reg, s->clip, s->S_cate, s->dense, s->dense_KT,
                                      s->dims_full, s->step_dev, s->loss_out, s->gnorm_out, s->opt, stream)))
      return rc;
  }
  if (phases & TLSAN_PHASE_APPLY) {
    if ((rc = tlsan_shard_apply_lazy_static(const_cast<float*>(s->shard), s->ld, s->cI, s->R, s->W, s->reg_item, s->reg_user, s->vals,
                                            s->ldv, s->recv_rows, s->cap, s->G, s->slots64, s->stamp, s->marked, s->gscale,
                                            s->step_dev, s->cate_emb, s->C, s->dc, s->g_cate, s->sumsq_out, s->sumsq_f32, s->scale,
                                            s->lws, s->lws_bytes, stream)))
      return rc;
  }
  if (plans && n_plans > 0 && (phases & TLSAN_PLAN_ASYNC)) {
    if (s->out.started == nullptr) return fail(TLSAN_E_BADARG, "TLSAN_PLAN_ASYNC needs the started word (out.started)");
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(g_pm);
    if (!g_pstarted) {
      std::thread(plan_worker).detach();
      g_pstarted = true;
    }
    for (int k = 0; k < n_plans; ++k) {
      if (!plans[k]) continue;
      PlanJob j;
      j.p = *plans[k]; j.dims = *plans[k]->dims; j.cp = *plans[k]->cp; j.cb = *plans[k]->cb;
      j.word = (volatile uint32_t*)s->out.started; j.after = s->plans_after; j.device = dev;
      g_pq.push_back(j);
    }
    g_pcv.notify_one();
  } else if (plans && n_plans > 0) {
    // The plans go to slots that earlier steps were the last to use: wait (on the host) until the pinned word says that
    // step `plans_after` has started -- everything queued before that step is then complete.  No event on the main stream.
    if (s->out.started != nullptr && !wait_started((volatile uint32_t*)s->out.started, s->plans_after))
      return fail(TLSAN_E_LAUNCH, "tlsan_shard_step_static: step %u did not start within 30 s", s->plans_after);
    for (int k = 0; k < n_plans; ++k)
      if (plans[k] && (rc = tlsan_shard_plan_static(plans[k]))) return rc;
  }
  return TLSAN_OK;
}

}  // extern "C"

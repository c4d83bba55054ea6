// tlsan_api.hip -- the core of the C ABI declared in include/tlsan.h: layout and sizes, the persistent state, the forward,
// the batch pack and index, the train step, tlsan_grads and the profiling ring: argument checking, workspace carving and
// kernel sequencing.  What a step builds and launches is decided in tlsan_api_plan.hip (tlsan_plan.h); this unit issues it.
// (Evaluation: tlsan_api_eval.hip; rows and the sharded step: tlsan_api_shard.hip; what they share: tlsan_host.h.)  No allocation, no synchronisation; everything is enqueued on the caller's stream (so a whole
// step can be captured into a hipGraph).
#include <stdarg.h>
#include <stdio.h>

#include <mutex>
#include <unordered_set>

#include "tlsan_plan.h"
#include "tlsan_index.h"
#include "tlsan_finalize.h"
#include "tlsan_apply.h"
#include "tlsan_update_lazy.h"
#include "tlsan_update_adagrad.h"

// ---- the small kernels of the dense side that only this unit launches
// (tlsan_state_renorm: the sum of squares must be complete before it is rescaled)
__global__ __launch_bounds__(256) void k_fold_delta(const DeltaRec* S_delta, int nrec, StateHdr* hdr, double* S_total) {
  __shared__ double shd[256];
  fold_delta(S_delta, nrec, hdr, S_total, shd);
}

// dedup-norm mode: norm^2 = sum over destination rows of |summed row gradient|^2 (ROWNORM pass)
// + dense gradients; overrides the coefficient / norm of the step summary
__global__ __launch_bounds__(256) void k_clip_dedup(const double* rown_part, int nrow, const float* sqd, int nsqd,
                                                    StateHdr* hdr, float clip, float* out_gnorm) {
  __shared__ double shd[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = tid; k < nrow; k += 256) s += rown_part[k];
  for (int k = tid; k < nsqd; k += 256) s += (double)sqd[k];
  shd[tid] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) shd[tid] += shd[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float norm = (float)sqrt(shd[0]);
    hdr->coef = clip_coef(norm, clip);
    if (out_gnorm) *out_gnorm = norm;
  }
}

__global__ __launch_bounds__(256) void k_reduce_double(const double* v, int n, double* out) {
  __shared__ double shd[256];
  const double s = block_sum_double(v, n, shd);
  if (threadIdx.x == 0) *out = s;
}

__global__ void k_transpose_K(const float* __restrict__ K, float* __restrict__ KT, int D) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < D * D) KT[(size_t)(t % D) * D + t / D] = K[t];
}

static thread_local char g_err[512] = "";   // (static: fail() and tlsan_last_error() are its only doors, for every unit)
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ---- profiling ring (tlsan_profile_*): events at the kernel boundaries of a train step ----
#define PROF_MAX_STEPS 4096
#define PROF_MARKS 6
static unsigned long long* g_stamps = nullptr;
#define TLSAN_APPLY_STAMP_OFF (1 << 20)  // k_apply's stamps start this many entries into the debug buffer
static int g_prof_level = 0;
static int g_prof_n = 0;
static int g_prof_stride = 1;  // record every g_prof_stride-th step (tlsan_profile_stride)
static int g_prof_tick = 0;    // steps seen since the ring was enabled
static hipEvent_t* g_prof_ev = nullptr;  // [PROF_MAX_STEPS][PROF_MARKS], created on first enable
static void prof_mark(int mark, hipStream_t hs) {
  // (the sampled step of every stride is the middle one: not the first step after the caller's fence, whose kernel
  //  starts on an idle GPU and runs 5-8 % longer than the others)
  if (g_prof_level == 0 || g_prof_n >= PROF_MAX_STEPS || (g_prof_tick % g_prof_stride) != g_prof_stride / 2) return;
  if (g_prof_level == 1) return;   // (the kernel's own events: prof_kernel_events)
  (void)hipEventRecord(g_prof_ev[g_prof_n * PROF_MARKS + mark], hs);
}

// level 1 (the fused kernel's own duration): the two events ride on the kernel's dispatch packet (hipExtLaunchKernelGGL) --
// its begin / end time stamps, what a kernel trace reports -- instead of being recorded around it as barrier packets of
// their own, which read ~3 us longer and delay the step that carries them
static LaunchEvents prof_kernel_events() {
  LaunchEvents ev = {nullptr, nullptr};
  if (g_prof_level != 1 || g_prof_n >= PROF_MAX_STEPS || (g_prof_tick % g_prof_stride) != g_prof_stride / 2) return ev;
  ev.start = g_prof_ev[g_prof_n * PROF_MARKS + 1];
  ev.stop = g_prof_ev[g_prof_n * PROF_MARKS + 2];
  return ev;
}

static void prof_step_done() {
  if (g_prof_level == 0) return;
  if ((g_prof_tick % g_prof_stride) == g_prof_stride / 2 && g_prof_n < PROF_MAX_STEPS) ++g_prof_n;
  ++g_prof_tick;
}

// The (d, heads) pairs of this build: their geometry and the launchers of their units (tlsan_attn_d*.hip, tlsan_update_d*.hip).
// (a pair is built when dh is 8, 16 or 32 and a sample spans 4 or 8 columns of max(dh, 16) channels: a sample's 4 * CPS
//  lanes cover its Ls + 3 use slots, and a pass of 16 samples is one workgroup of CPS wavefronts -- Geo)
struct Pair {
  int D, DH, NSB, NPB, CW;
  hipError_t (*fwd_bwd)(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
  void (*finalize)(const FinLaunch& L, hipStream_t hs);
  // optional: a training kernel of smaller workgroups for small batches, and its samples per pass (Shape::SG; when it is
  // taken: FrontPlan::small, tlsan_api_plan.hip)
  hipError_t (*fwd_bwd_small)(const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
  int small_grp;
};
#define PAIR(D, DH, U, ...) {D, DH, Geo<D, DH>::NSB, Geo<D, DH>::NPB, Geo<D, DH>::CW, tlsan_launch_fwd_bwd_##U, tlsan_launch_finalize_##U, __VA_ARGS__}
static const Pair g_pairs[] = {PAIR(64, 8, d64),      PAIR(64, 16, d64h4),   PAIR(128, 16, d128, tlsan_launch_fwd_bwd_d128w4, 8),
                               PAIR(128, 8, d128h16), PAIR(128, 32, d128h4), PAIR(256, 32, d256)};
#undef PAIR
static const Pair* pair_of(int D, int DH) {
  for (const Pair& pr : g_pairs)
    if (pr.D == D && pr.DH == DH) return &pr;
  return nullptr;
}

int shape_of(const tlsan_dims* d, Shape* s) {
  if (!d) return fail(TLSAN_E_BADARG, "dims is NULL");
  if (d->num_heads <= 0 || d->d % d->num_heads) return fail(TLSAN_E_BADARG, "d %% num_heads != 0");
  const int D = d->d, DH = D / d->num_heads;
  if (d->d_item + d->d_cate != D) return fail(TLSAN_E_BADARG, "d_item + d_cate != d (model.py:100-109)");
  if (d->d_item % 4 || d->d_cate % 4 || d->d_item > 128 || d->d_cate > 128)
    return fail(TLSAN_E_UNSUPPORTED, "embedding widths must be multiples of 4 and <= 128");
  if (d->Ls < 1 || d->Ls > TLSAN_LS_CAP) return fail(TLSAN_E_UNSUPPORTED, "Ls must be in 1..%d", TLSAN_LS_CAP);
  if (d->user_count < 1 || d->item_count < 1 || d->cate_count < 1) return fail(TLSAN_E_BADARG, "empty table");
  s->D = D;
  s->DH = DH;
  const Pair* pr = pair_of(D, DH);
  if (!pr) return fail(TLSAN_E_UNSUPPORTED, "unsupported (hidden_units=%d, num_heads=%d): this build has (hidden_units, num_heads) = "
                       "64/4, 64/8, 128/4, 128/8, 128/16, 256/8", D, d->num_heads);
  s->NSB = pr->NSB; s->NPB = pr->NPB; s->CW = pr->CW; s->SG = pr->small_grp;
  return TLSAN_OK;
}

int check_params(const tlsan_params* p) {
  if (!p || !p->item_emb || !p->item_b || !p->user_emb || !p->usert_emb || !p->cate_emb || !p->dense ||
      !p->dense_KT || !p->item_cate)
    return fail(TLSAN_E_BADARG, "NULL parameter pointer");
  if (p->table_dtype != TLSAN_TABLE_F32 && p->table_dtype != TLSAN_TABLE_BF16) return fail(TLSAN_E_BADARG, "table_dtype");
  if (p->matrix_dtype != TLSAN_MATRIX_F32 && p->matrix_dtype != TLSAN_MATRIX_BF16) return fail(TLSAN_E_BADARG, "matrix_dtype");
  if (p->table_dtype == TLSAN_TABLE_BF16 && ((p->ld_item | p->ld_user) % 4))
    return fail(TLSAN_E_UNSUPPORTED, "bf16 tables need row strides that are multiples of 4 elements");
  return TLSAN_OK;
}

static int ru4(int x) { return (x + 3) / 4 * 4; }
void carve(const tlsan_dims* d, const Shape& s, int B, int Sn, char* base, Ws* w) {
  size_t o = 0;
  auto take = [&](size_t n) { char* p = base ? base + o : nullptr; o += al(n); return p; };
  const size_t NI = (size_t)B * (d->Ls + Sn + 1), D = s.D;
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  const Capacity cap = plan_capacity(d, s, B);
  w->WU = ru4(d->d_item + d->Ls);
  w->nbK = (s.D * s.D + 255) / 256;
  const int small_pb = s.D > 128 ? FIN_SMALL_PB : 16;      // (small parameters per finalize workgroup: dense_finalize_block)
  w->nbS = (L.n_dense - s.D * s.D + small_pb - 1) / small_pb;
  w->nfin = w->nbK + w->nbS;
  // (+1 row: k_apply reads clamped addresses instead of branching, see AP_OWN)
  w->Gi = (float*)take(sizeof(float) * (NI + 1) * D);
  w->Gb = (float*)take(sizeof(float) * (NI + 1));
  w->Gu = (float*)take(sizeof(float) * (size_t)(B + 1) * w->WU);
  w->Gc = (float*)take(sizeof(float) * (size_t)(B + 1 + (cap.cseg ? NI : 0)) * d->d_cate);
  w->gLong = (float*)take(sizeof(float) * B * D);
  w->gDB = (float*)take(sizeof(float) * B * D);
  // windows too long for the registers (cap.lstream) with two 16-channel blocks per column (d = 256, and d = 128 with
  // 4 heads): per-sample softmax statistics of the long block (k_fwd_bwd, FLATG: no room in the LDS)
  w->gStat = (float*)take((s.CW > 16 && cap.lstream) ? sizeof(float) * (size_t)B * 2 * D : 0);
  w->partials = (float*)take(sizeof(float) * cap.max_records * s.NPB);
  w->Kp = (float*)take(sizeof(float) * cap.kp_slots * D * D);
  w->gd = (float*)take(sizeof(float) * L.n_dense);
  w->sqd = (float*)take(sizeof(float) * w->nfin);
  w->scal = (float*)take(sizeof(float) * 4);
  w->logits = (float*)take(sizeof(float) * B);
  w->s_label = (float*)take(sizeof(float) * B);
  {
    const size_t ae = sizeof(float) * (size_t)d->item_count * D;
    w->all_emb = ae <= EVAL_DENSE_MAX ? (float*)take(ae) : nullptr;
  }
  const size_t nrowblk = (size_t)(d->item_count + 15) / 16 + (d->user_count + 15) / 16 + d->cate_count;
  {  // summed rows of the used rows (lazy update: k_finalize_presum -> k_update_lazy)
    const size_t ri = (NI < (size_t)d->item_count ? NI : (size_t)d->item_count) + AP_ROWS_PB;
    const size_t ru = ((size_t)B < (size_t)d->user_count ? (size_t)B : (size_t)d->user_count) + AP_ROWS_PB;
    w->Ri = (float*)take(sizeof(float) * ri * d->d_item);
    w->Rb = (float*)take(sizeof(float) * ri);
    w->Ru = (float*)take(sizeof(float) * ru * w->WU);
    w->Rc = (float*)take(sizeof(float) * (size_t)d->cate_count * d->d_cate);
  }
  w->rownorm_part = (double*)take(8 * nrowblk);
  w->rownorm = (double*)take(8);
  w->bytes = o;
}

// a table of more scan blocks (chunks of 4096 rows) than SCAN_TWO_LEVEL_BLOCKS: the scan's two-launch form
static bool scan_two_level(const int32_t n[3]) {
  for (int k = 0; k < 3; ++k)
    if ((n[k] + 4095) / 4096 > SCAN_TWO_LEVEL_BLOCKS) return true;
  return false;
}
// exclusive scans of up to three count arrays in one launch (two for large tables, see k_index_scan);
// bsum: scratch of >= nscan packed sums, or NULL (then always the single launch)
int launch_scan(ScanArgs& sa, int nscan, long long* bsum, hipStream_t hs) {
  const bool big = scan_two_level(sa.n);
  sa.bsum = nullptr;
  if (big && bsum) {
    sa.bsum = bsum;
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nscan), dim3(1024), 0, hs, sa);
    CHECK_LAUNCH("k_scan_block_sums");
  }
  sa.bal.blk = nscan;
  sa.us.blk = nscan + (sa.bal.perm ? 1 : 0);
  sa.is.blk = sa.us.blk + (sa.us.u ? 1 : 0);       // (the finishing blocks of the item side's counting sort come last)
  hipLaunchKernelGGL(k_index_scan, dim3(sa.is.blk + (sa.is.on ? sa.is.nfin : 0)), dim3(1024), 0, hs, sa);
  CHECK_LAUNCH("k_index_scan");
  return TLSAN_OK;
}

int scan_compact_impl(const int32_t* cnt, int32_t n, int32_t* prefix, int32_t* uniq, int32_t* n_uniq, long long* bsum,
                             hipStream_t hs) {
  if (!cnt || !prefix || n < 1) return fail(TLSAN_E_BADARG, "tlsan_scan_compact: bad arguments");
  ScanArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.cnt[0] = cnt; sa.off[0] = prefix; sa.cur[0] = nullptr; sa.n[0] = n;
  sa.uniq[0] = uniq; sa.n_uniq[0] = n_uniq;
  const int nscan = (n + 4095) / 4096;
  sa.blk0[0] = 0; sa.blk0[1] = nscan; sa.blk0[2] = nscan;
  return launch_scan(sa, nscan, bsum, hs);
}

int launch_reduce_double(const double* v, int n, double* out, hipStream_t hs) {
  hipLaunchKernelGGL(k_reduce_double, dim3(1), dim3(256), 0, hs, v, n, out);
  CHECK_LAUNCH("k_reduce_double");
  return TLSAN_OK;
}

struct St {  // persistent state
  // two index slots (a batch's destination index depends only on its ids, so it lives with the
  // state, not in the per-call workspace whose layout follows the batch shape):
  int32_t *cnt_item[TLSAN_INDEX_SLOTS], *cnt_uc[TLSAN_INDEX_SLOTS], *cnt_user[TLSAN_INDEX_SLOTS];   // use counters, zero at rest
  int32_t *off_item[TLSAN_INDEX_SLOTS], *off_uc[TLSAN_INDEX_SLOTS], *off_user[TLSAN_INDEX_SLOTS];   // segment offsets (n+1 entries)
  int32_t *cur_item[TLSAN_INDEX_SLOTS], *cur_uc[TLSAN_INDEX_SLOTS], *cur_user[TLSAN_INDEX_SLOTS];   // fill cursors
  int4 *urec_item[TLSAN_INDEX_SLOTS], *urec_user[TLSAN_INDEX_SLOTS];   // (row, first position, uses) of the used rows
  int32_t *cate_off, *cate_cnt, *cate_cur, *cate_items;   // static CSR category -> items
  StateHdr* hdr;
  double *S_part, *S_total;
  DeltaRec* S_delta;                                      // per-workgroup changes of the sum of squares, tagged by step (tlsan_state.h)
  long long* scan_bsum[TLSAN_INDEX_SLOTS];                                // per-chunk sums of the index scan (large tables), per slot
  int32_t* perm[TLSAN_INDEX_SLOTS];                                       // samples of every workgroup of the fused kernel (BalArgs), Capacity::rank_cap each
  int32_t* scan_ticket;                                                   // [index slot] arrivals of k_scan_block_sums (ScanArgs.bs_ticket), zero at rest
  int32_t* flag_user[TLSAN_INDEX_SLOTS];                                  // 256-row pieces of the user table that hold a count (ScanArgs.flag), zero at rest
  int32_t* uc_list[TLSAN_INDEX_SLOTS];                                    // samples of every category (u_cate uses), Capacity::uc_list_cap each
  double* Rc64;                                           // category sums of a split PRESUM pass, zero at rest
  int32_t* hot_list[TLSAN_INDEX_SLOTS];                                   // slots (urec_item) of the hot item rows, AP_HOT_CAP each
  // the item side of the index from a partitioned counting sort of the batch's ids (IsortArgs; where Capacity::isort says so)
  int32_t *is_bh[TLSAN_INDEX_SLOTS], *is_ids[TLSAN_INDEX_SLOTS], *is_bstart[TLSAN_INDEX_SLOTS], *is_nd[TLSAN_INDEX_SLOTS];
  int4* is_tmp[TLSAN_INDEX_SLOTS];
  void* fix_args;   // the ApplyArgs of the last two-launch step (k_finalize_update leaves them; spec_fix_blocks reads them)
  size_t bytes;
  int nbI, nbU, nbC;
  int nrec;   // records per step-parity array of S_delta: a workgroup each of the row blocks and the hot-row workgroups
};

static void carve_state(const tlsan_dims* d, const Shape& shp, char* base, St* s) {
  const Capacity cap = plan_capacity(d, shp, 1);   // (the state's answers do not depend on the batch)
  size_t o = 0;
  // (a NULL base leaves every pointer as its byte offset into the state: tlsan_state_bytes, tlsan_index_layout_of)
  auto take = [&](size_t n) { char* p = base + o; o += al(n); return p; };
  s->nbI = (d->item_count + AP_ROWS_PB - 1) / AP_ROWS_PB;
  s->nbU = (d->user_count + AP_ROWS_PB - 1) / AP_ROWS_PB;
  s->nbC = d->cate_count;
  s->hdr = (StateHdr*)take(sizeof(StateHdr));  // must stay first: tlsan_state_scale(state) == state
  for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k) {
    s->cnt_item[k] = (int32_t*)take(4 * (size_t)d->item_count);
    s->cnt_uc[k] = (int32_t*)take(4 * (size_t)d->cate_count);
    s->cnt_user[k] = (int32_t*)take(4 * (size_t)d->user_count);
    s->off_item[k] = (int32_t*)take(4 * ((size_t)d->item_count + 1));
    s->off_uc[k] = (int32_t*)take(4 * ((size_t)d->cate_count + 1));
    s->off_user[k] = (int32_t*)take(4 * ((size_t)d->user_count + 1));
    s->cur_item[k] = (int32_t*)take(4 * (size_t)d->item_count);
    s->cur_uc[k] = (int32_t*)take(4 * (size_t)d->cate_count);
    s->cur_user[k] = (int32_t*)take(4 * (size_t)d->user_count);
    s->urec_item[k] = (int4*)take(16 * ((size_t)d->item_count + AP_ROWS_PB));
    s->urec_user[k] = (int4*)take(16 * ((size_t)d->user_count + AP_ROWS_PB));
  }
  s->cate_off = (int32_t*)take(4 * (size_t)d->cate_count);
  s->cate_cnt = (int32_t*)take(4 * (size_t)d->cate_count);
  s->cate_cur = (int32_t*)take(4 * (size_t)d->cate_count);
  s->cate_items = (int32_t*)take(4 * (size_t)d->item_count);
  s->S_part = (double*)take(8 * (size_t)(s->nbI + s->nbU + s->nbC));
  s->nrec = s->nbI + s->nbU + s->nbC + AP_HOT_CAP;
  s->S_delta = (DeltaRec*)take(sizeof(DeltaRec) * 2 * (size_t)s->nrec);   // (two arrays, by step parity: DeltaRec)
  for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k) s->uc_list[k] = (int32_t*)take(4 * (size_t)cap.uc_list_cap);
  s->Rc64 = (double*)take(8 * (size_t)d->cate_count * d->d_cate);
  for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k) s->hot_list[k] = (int32_t*)take(4 * (size_t)AP_HOT_CAP);
  for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k)
    s->scan_bsum[k] = (long long*)take(8 * ((size_t)(d->item_count + 4095) / 4096 + (d->cate_count + 4095) / 4096 +
                                            (d->user_count + 4095) / 4096));
  for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k) s->perm[k] = (int32_t*)take(4 * (size_t)cap.rank_cap);
  s->scan_ticket = (int32_t*)take(4 * 64);
  for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k) s->flag_user[k] = (int32_t*)take(4 * (((size_t)d->user_count + 255) / 256));
  {
    const bool on = cap.isort;
    for (int k = 0; k < TLSAN_INDEX_SLOTS; ++k) {
      s->is_bh[k] = (int32_t*)take(on ? 4 * (size_t)(ISORT_MAX_SLOTS / IS_BLK_SLOTS) * IS_MAXB : 0);
      s->is_ids[k] = (int32_t*)take(on ? 4 * (size_t)ISORT_MAX_SLOTS : 0);
      s->is_bstart[k] = (int32_t*)take(on ? 4 * (size_t)(IS_MAXB + 1) : 0);
      s->is_nd[k] = (int32_t*)take(on ? 4 * (size_t)IS_MAXB : 0);
      s->is_tmp[k] = (int4*)take(on ? 16 * (size_t)ISORT_MAX_SLOTS : 0);
    }
  }
  s->fix_args = take(sizeof(ApplyArgs));
  s->S_total = base ? &s->hdr->St : nullptr;
  s->bytes = o;
}

static bool two_listed(const void* state, bool remove);   // (the states that may owe a correction: below, at tlsan_state_flush)

extern "C" {

int tlsan_abi_version(void) { return TLSAN_ABI_VERSION; }
const char* tlsan_last_error(void) { return g_err; }

int tlsan_dense_layout_of(const tlsan_dims* d, tlsan_dense_layout* L) {
  if (!d || !L || d->num_heads <= 0) return fail(TLSAN_E_BADARG, "null dims/layout");
  const int D = d->d, dh = D / d->num_heads;
  int o = 0;
  L->f1_W1 = o; o += dh * dh;
  L->f1_b1 = o; o += dh;
  L->f1_W2 = o; o += dh * dh;
  L->f1_b2 = o; o += dh;
  L->K = o; o += D * D;
  L->k0 = o; o += D;
  L->f2_W1 = o; o += dh * dh;
  L->f2_b1 = o; o += dh;
  L->f2_W2 = o; o += dh * dh;
  L->f2_b2 = o; o += dh;
  L->gamma = o; o += 1;
  L->n_dense = o;
  return TLSAN_OK;
}

size_t tlsan_workspace_bytes(const tlsan_dims* d, int32_t max_B, int32_t max_Sn) {
  Shape s;
  if (shape_of(d, &s) != TLSAN_OK || max_B < 1 || max_Sn < 0) return 0;
  Ws w;
  carve(d, s, max_B, max_Sn, nullptr, &w);
  return w.bytes;
}

size_t tlsan_state_bytes(const tlsan_dims* d) {
  Shape s;
  if (shape_of(d, &s) != TLSAN_OK) return 0;
  St st;
  carve_state(d, s, nullptr, &st);
  return st.bytes;
}

static int check_batch(const tlsan_dims* d, const tlsan_batch* b, bool train) {
  if (!b || b->B < 1 || b->Sn < 0) return fail(TLSAN_E_BADARG, "bad batch (B=%d, Sn=%d)", b ? b->B : -1, b ? b->Sn : -1);
  if (!b->u || !b->i || !b->hist_i || !b->hist_t || !b->sl || !b->sl_new || !b->u_cate || (b->Sn > 0 && !b->hist_i_new))
    return fail(TLSAN_E_BADARG, "NULL batch pointer");
  if (train && !b->y) return fail(TLSAN_E_BADARG, "training needs labels y");
  if ((size_t)b->B * (d->Ls + b->Sn + 2) >= ((size_t)1 << 31)) return fail(TLSAN_E_UNSUPPORTED, "B*S overflows int32");
  if (train && b->Sn > TLSAN_SN_CAP) return fail(TLSAN_E_UNSUPPORTED, "training supports sessions up to %d items (got Sn=%d)", TLSAN_SN_CAP, b->Sn);
  return TLSAN_OK;
}

// ix: the plan of the batch's index; NULL where there is no batch (recompute_sumsq)
static void fill_apply(ApplyArgs& A, const tlsan_dims* d, const Shape& s, const tlsan_params* p, const IndexPlan* ix,
                       const tlsan_hparams* hp, const Ws& w, const St& st, const tlsan_dense_layout& L) {
  const int k = hp ? hp->index_slot : 0;
  memset(&A, 0, sizeof(A));
  A.p = norm_params(p, d);
  A.lay = L;
  A.I = d->item_count; A.U = d->user_count; A.C = d->cate_count; A.Ls = d->Ls; A.D = s.D;
  A.di = d->d_item; A.dc = d->d_cate; A.WU = ru4(d->d_item + d->Ls);
  A.Gi = w.Gi; A.Gb = w.Gb; A.Gu = w.Gu; A.Gc = w.Gc;
  A.cnt_item = st.cnt_item[k]; A.cnt_uc = st.cnt_uc[k]; A.cnt_user = st.cnt_user[k];
  A.off_item = st.off_item[k]; A.off_uc = st.off_uc[k]; A.off_user = st.off_user[k];
  A.n_uniq_item = st.hdr ? &st.hdr->n_uniq[k][0] : nullptr; A.n_uniq_user = st.hdr ? &st.hdr->n_uniq[k][1] : nullptr;
  A.cate_off = st.cate_off; A.cate_cnt = st.cate_cnt; A.cate_items = st.cate_items;
  A.uc_list = (ix && ix->uc_list) ? st.uc_list[k] : nullptr;
  A.cseg = (ix && ix->cseg) ? 1 : 0;
  A.Rc64 = st.Rc64;
  A.csplit = 1; A.cpass = 256; A.cpos = 0;
  A.hot_n = st.hdr ? &st.hdr->n_hot[k] : nullptr; A.hot_list = st.hot_list[k];
  A.gd = w.gd;
  A.Rc = w.Rc; A.Ri = w.Ri; A.Rb = w.Rb; A.Ru = w.Ru;
  A.part_out = st.S_part; A.delta_out = st.S_delta; A.delta_nrec = st.nrec; A.hdr = st.hdr;
  A.fix_args = st.fix_args;   // (plan_tail keeps it for the two-launch form only)
  A.urec_item = st.urec_item[k]; A.urec_user = st.urec_user[k];
  if (hp) { A.lr = hp->lr; A.reg = hp->reg; }
  A.nbI = st.nbI; A.nbU = st.nbU; A.nbC = st.nbC; A.nbD = (L.n_dense + 255) / 256;
  if (A.cseg) A.nbC = (A.C + AP_ROWS_PB - 1) / AP_ROWS_PB;     // (16 categories per workgroup: apply_cseg_block)
  A.stamps = g_stamps ? g_stamps + TLSAN_APPLY_STAMP_OFF : nullptr;
}

// one apply pass = one launch: category rows, item/user rows (+ dense parameters).
static int launch_apply(int mode, ApplyArgs A, bool with_dense, hipStream_t hs) {
  const dim3 g1(A.nbC + A.nbI + A.nbU + (with_dense ? A.nbD : 0)), blk(256);
  const bool wide = apply_wide(A);
  const bool bf16 = A.p.table_dtype == TLSAN_TABLE_BF16;
#define AP_LAUNCH(M)                                                                                         \
  do {                                                                                                       \
    if (bf16) {                                                                                              \
      if (wide) hipLaunchKernelGGL((k_apply<M, true, TLSAN_TABLE_BF16>), g1, blk, 0, hs, A);                 \
      else hipLaunchKernelGGL((k_apply<M, false, TLSAN_TABLE_BF16>), g1, blk, 0, hs, A);                     \
    } else {                                                                                                 \
      if (wide) hipLaunchKernelGGL((k_apply<M, true>), g1, blk, 0, hs, A);                                   \
      else hipLaunchKernelGGL((k_apply<M, false>), g1, blk, 0, hs, A);                                       \
    }                                                                                                        \
  } while (0)
  switch (mode) {
    case AP_UPDATE: AP_LAUNCH(AP_UPDATE); break;
    case AP_GRADS: AP_LAUNCH(AP_GRADS); break;
    case AP_SUMSQ: AP_LAUNCH(AP_SUMSQ); break;
    default: AP_LAUNCH(AP_ROWNORM); break;
  }
#undef AP_LAUNCH
  CHECK_LAUNCH("k_apply");
  return TLSAN_OK;
}

int tlsan_sync_derived(const tlsan_dims* d, const tlsan_params* p, void* stream) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_transpose_K, dim3((s.D * s.D + 255) / 256), dim3(256), 0, st, p->dense + L.K, p->dense_KT, s.D);
  CHECK_LAUNCH("k_transpose_K");
  return TLSAN_OK;
}

// the opening of the four tlsan_state_* calls: the checks, then the state's carve-up
static int open_state(const tlsan_dims* d, const tlsan_params* p, void* state, Shape* s, St* st) {
  int rc = shape_of(d, s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  if (!state) return fail(TLSAN_E_WORKSPACE, "state is NULL");
  carve_state(d, *s, (char*)state, st);
  return TLSAN_OK;
}

static int cate_csr(const tlsan_dims* d, const tlsan_params* p, const St& st, hipStream_t hs) {
  return build_cate_csr(p->item_cate, d->item_count, d->cate_count, st.cate_cnt, st.cate_off, st.cate_cur, st.cate_items, hs);
}

// the sum of squares of the four stored tables, from what is stored
static int recompute_sumsq(const tlsan_dims* d, const Shape& s, const tlsan_params* p, const St& st, hipStream_t hs) {
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  Ws w;
  memset(&w, 0, sizeof(w));
  ApplyArgs A;
  fill_apply(A, d, s, p, nullptr, nullptr, w, st, L);
  int rc = launch_apply(AP_SUMSQ, A, false, hs);
  if (rc) return rc;
  if ((rc = launch_reduce_double(st.S_part, st.nbI + st.nbU + st.nbC, st.S_total, hs))) return rc;
  // (per-step CHANGES of the sum travel as tagged records in S_delta, folded by the next step's k_dense_finalize)
  if (hipMemsetAsync(st.S_part, 0, 8 * (size_t)(st.nbI + st.nbU + st.nbC), hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "memset S_part");
  return TLSAN_OK;
}

int tlsan_state_init(const tlsan_dims* d, const tlsan_params* p, void* state, void* stream) {
  Shape s; St st;
  int rc = open_state(d, p, state, &s, &st);
  if (rc) return rc;
  if ((rc = tlsan_sync_derived(d, p, stream))) return rc;
  hipStream_t hs = (hipStream_t)stream;
  two_listed(state, true);   // (a fresh state owes nothing)
  if (hipMemsetAsync(state, 0, st.bytes, hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "memset state");
  static const float one = 1.0f;  // table scale P = 1
  if (hipMemcpyAsync(&st.hdr->P, &one, sizeof(float), hipMemcpyHostToDevice, hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "init P");
  if ((rc = cate_csr(d, p, st, hs))) return rc;
  return recompute_sumsq(d, s, p, st, hs);
}

const float* tlsan_state_scale(const void* state) { return (const float*)state; }

// The states whose last training step took the two-launch form: a clipped one may still owe its correction
// (StateHdr::fix_pending), which the next step of that form makes at the head of its fused kernel.  Every other call that
// reads or rewrites the tables, the dense parameters or that step's index slot flushes first -- a launch, so only for the
// states in this set.  (A hint, not the truth: the truth is the header's word, and a flush of a state that owes nothing
// returns at once.  The set has no limit; a state leaves it when it is flushed or initialised, so a state that is freed
// without either leaves its eight bytes behind.  Replayed graphs pass the host by: see step_flush.)
static std::mutex g_two_mu;
static std::unordered_set<const void*> g_two_states;
static bool two_listed(const void* state, bool remove) {
  std::lock_guard<std::mutex> lk(g_two_mu);
  return remove ? g_two_states.erase(state) != 0 : g_two_states.count(state) != 0;
}
static void two_list(const void* state) {
  std::lock_guard<std::mutex> lk(g_two_mu);
  g_two_states.insert(state);
}
static int flush_state(const tlsan_dims* d, const tlsan_params* p, const St& st, hipStream_t hs) {
  tlsan_launch_spec_flush(apply_wide(d->d_item, d->d_cate, ru4(d->d_item + d->Ls)), p->table_dtype == TLSAN_TABLE_BF16, st.fix_args, st.hdr, hs);
  CHECK_LAUNCH("k_spec_flush");
  return TLSAN_OK;
}
static int flush_if_listed(const tlsan_dims* d, const tlsan_params* p, void* state, const St& st, hipStream_t hs) {
  return two_listed(state, true) ? flush_state(d, p, st, hs) : TLSAN_OK;
}
static bool capturing(hipStream_t hs) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(hs, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
// The flush in front of a training step.  A two-launch step whose index was built ahead makes the correction at the head of
// its fused kernel and needs none.  Every other step needs it if the state owes (a two-launch step that builds its own
// index too: the correction walks its step's slot, which the build overwrites).  A graph replays what was recorded, not
// what the set said on the day of the capture, and the state may owe at any replay: a two-launch step that is being
// captured records the flush always (it returns at once on the device when nothing is owed).
static int step_flush(const tlsan_dims* d, const tlsan_params* p, void* state, const St& st, hipStream_t hs, bool two, bool prebuilt) {
  if (two && prebuilt) return TLSAN_OK;
  if (two && capturing(hs)) { two_listed(state, true); return flush_state(d, p, st, hs); }
  return flush_if_listed(d, p, state, st, hs);
}

int tlsan_state_flush(const tlsan_dims* d, const tlsan_params* p, void* state, void* stream) {
  Shape s; St st;
  int rc = open_state(d, p, state, &s, &st);
  if (rc) return rc;
  hipStream_t hs = (hipStream_t)stream;
  two_listed(state, true);
  if ((rc = flush_state(d, p, st, hs)) || capturing(hs)) return rc;
  // StateHdr::fix_failed: a fused kernel gave up its bounded wait for the correcting workgroups (spec_fix_head) and left the
  // scale NaN.  The device cannot reach the host's error word; this call, which its callers make before they read, can.
  uint32_t failed = 0;
  if (hipMemcpyAsync(&failed, &st.hdr->fix_failed, sizeof(failed), hipMemcpyDeviceToHost, hs) != hipSuccess ||
      hipStreamSynchronize(hs) != hipSuccess)
    return fail(TLSAN_E_LAUNCH, "tlsan_state_flush: reading the state's header");
  if (failed) return fail(TLSAN_E_LAUNCH, "a training step gave up waiting for a clipped step's correction: the table scale is NaN (tlsan_state_init starts over)");
  return TLSAN_OK;
}

int tlsan_state_renorm(const tlsan_dims* d, const tlsan_params* p, void* state, void* stream) {
  Shape s; St st;
  int rc = open_state(d, p, state, &s, &st);
  if (rc) return rc;
  const tlsan_params q = norm_params(p, d);
  hipStream_t hs = (hipStream_t)stream;
  if ((rc = flush_if_listed(d, p, state, st, hs))) return rc;
  const int dt = q.table_dtype;
  // (changes of the sum of squares the last update left as records: part of St before St is rescaled)
  hipLaunchKernelGGL(k_fold_delta, dim3(1), dim3(256), 0, hs, st.S_delta, st.nrec, st.hdr, st.S_total);
  hipLaunchKernelGGL(k_scale_table, dim3(1024), dim3(256), 0, hs, q.item_emb, d->item_count, d->d_item, q.ld_item, st.hdr, dt, 0x1b873593u);
  hipLaunchKernelGGL(k_scale_table, dim3(1024), dim3(256), 0, hs, q.user_emb, d->user_count, d->d_item, q.ld_user, st.hdr, dt, 0xcc9e2d51u);
  hipLaunchKernelGGL(k_scale_table, dim3(256), dim3(256), 0, hs, q.usert_emb, d->user_count, d->Ls, q.ld_usert, st.hdr, TLSAN_TABLE_F32, 0u);
  hipLaunchKernelGGL(k_scale_table, dim3(64), dim3(256), 0, hs, q.cate_emb, d->cate_count, d->d_cate, d->d_cate, st.hdr, dt, 0xe6546b64u);
  hipLaunchKernelGGL(k_renorm_commit, dim3(1), dim3(1), 0, hs, st.hdr);
  CHECK_LAUNCH("tlsan_state_renorm");
  // bf16 tables: the rounded values no longer scale exactly with P -- take the sum of squares from what is stored
  // (per-step changes still pending in S_part are already part of the stored values: overwritten)
  return dt != TLSAN_TABLE_F32 ? recompute_sumsq(d, s, p, st, hs) : TLSAN_OK;
}

int tlsan_state_reindex(const tlsan_dims* d, const tlsan_params* p, void* state, void* stream) {
  Shape s; St st;
  int rc = open_state(d, p, state, &s, &st);
  if (rc) return rc;
  hipStream_t hs = (hipStream_t)stream;
  if ((rc = flush_if_listed(d, p, state, st, hs))) return rc;   // (the correction walks the index this call clears)
  const size_t skip = al(sizeof(StateHdr));  // keep P / St
  if (hipMemsetAsync((char*)state + skip, 0, st.bytes - skip, hs) != hipSuccess) return fail(TLSAN_E_LAUNCH, "memset state");
  return cate_csr(d, p, st, hs);
}

int tlsan_state_recategorize(const tlsan_dims* d, const tlsan_params* p, void* state, void* stream) {
  Shape s; St st;
  const int rc = open_state(d, p, state, &s, &st);
  return rc ? rc : cate_csr(d, p, st, (hipStream_t)stream);
}

// the fused kernel as the plan says (a.ngroups, a.fuse_dk: the plan's as well)
static int launch_fwd(const Shape& s, bool train, const FrontPlan& fp, const FwdArgs& a, hipStream_t hs) {
  hipError_t e;
  LaunchEvents ev = {nullptr, nullptr};
  if (train) ev = prof_kernel_events();
  const Pair* pr = pair_of(s.D, s.DH);   // (shape_of has refused every other pair)
  if (fp.small) e = pr->fwd_bwd_small(a, fp.grid, hs, ev);
  else e = pr->fwd_bwd(train, fp.lstream, a, fp.grid, hs, ev);
  if (e == hipErrorNotSupported)
    return fail(TLSAN_E_UNSUPPORTED, "dropout > 0 is built for train steps only (and not for the 8-sample workgroup form)");
  if (e != hipSuccess) return fail(TLSAN_E_LAUNCH, "k_fwd_bwd: %s", hipGetErrorString(e));
  return TLSAN_OK;
}

static void fill_fwd(FwdArgs& a, const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, const FrontPlan& fp,
                     const tlsan_dense_layout& L) {
  memset(&a, 0, sizeof(a));
  a.p = norm_params(p, d);
  a.b = *b;
  a.lay = L;
  a.Ls = d->Ls; a.di = d->d_item; a.dc = d->d_cate;
  a.ngroups = fp.ngroups;
  a.fuse_dk = fp.fuse_dk ? 1 : 0;
  a.inv_B = 1.0f / (float)b->B;
  a.stamps = g_stamps;
}

int tlsan_forward(const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, float* logits_i, float* logits_j,
                  float* u_t, void* ws, size_t ws_bytes, void* stream) {
  return tlsan_forward_att(d, p, b, logits_i, logits_j, u_t, nullptr, nullptr, ws, ws_bytes, stream);
}

int tlsan_forward_att(const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, float* logits_i, float* logits_j,
                      float* u_t, float* att0, float* att1, void* ws, size_t ws_bytes, void* stream) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  if ((rc = check_batch(d, b, false))) return rc;
  (void)ws; (void)ws_bytes;
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  const FrontPlan fp = plan_forward(d, s, b);
  FwdArgs a;
  fill_fwd(a, d, p, b, fp, L);
  a.logits_i = logits_i;
  a.logits_j = logits_j;
  a.u_t = u_t;
  a.att0 = att0; a.att1 = att1;
  return launch_fwd(s, false, fp, a, (hipStream_t)stream);
}

// rows per table [item, category, user] that the index scan walks: a side that comes from a sort of the batch's ids has none
static void scanned_rows(const tlsan_dims* d, const IndexPlan& ix, int32_t n[3]) {
  n[0] = ix.isort ? 0 : d->item_count; n[1] = d->cate_count; n[2] = ix.usort ? 0 : d->user_count;
}

// destination index of a batch into slot k: use counts per destination row -> first sorted position
// of every row (+ records of the used rows)
static int build_index(const tlsan_dims* d, const tlsan_batch* b, const IndexPlan& ix, const int32_t* item_cate, const St& st,
                       int k, hipStream_t hs) {
  const bool cseg = ix.cseg, usort = ix.usort, isort = ix.isort;
  const int nthr = ix.nthr;
  if (cseg && !item_cate) return fail(TLSAN_E_BADARG, "tables with %d categories count item uses per category: item_cate is NULL", d->cate_count);
  int rc;
  CountArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.b = *b; ca.Ls = d->Ls;
  ca.n_hot = &st.hdr->n_hot[k];
  ca.cnt_item = st.cnt_item[k]; ca.cnt_user = st.cnt_user[k]; ca.cnt_uc = st.cnt_uc[k];
  ca.item_cate = cseg ? item_cate : nullptr; ca.cseg = cseg ? 1 : 0;
  ca.ncate = d->cate_count;
  ca.flag_user = st.flag_user[k];
  ca.skip_users = usort ? 1 : 0;
  ScanArgs sa;
  memset(&sa, 0, sizeof(sa));
  if (isort) {
    IsortArgs& ia = sa.is;
    ia.on = 1;
    ia.b = *b; ia.Ls = d->Ls;
    ia.nbu = (b->B + 1023) / 1024;   // (k_count's sample blocks: k_count does not run)
    ia.n = d->item_count;
    ia.shift = 0;   // few, full buckets: up to IS_BSZ ids each, at least 64 of them
    while (((ia.n - 1) >> ia.shift) >= IS_MAXB || ((1 << ia.shift) < IS_BSZ && ((ia.n - 1) >> ia.shift) >= 64)) ++ia.shift;
    ia.nb = ((ia.n - 1) >> ia.shift) + 1;
    ia.nslots = nthr;
    ia.nblk = (nthr + IS_BLK_SLOTS - 1) / IS_BLK_SLOTS;
    ia.bh = st.is_bh[k]; ia.ids = st.is_ids[k]; ia.bstart = st.is_bstart[k]; ia.nd = st.is_nd[k]; ia.tmp = st.is_tmp[k];
    ia.cur = st.cur_item[k]; ia.off = st.off_item[k]; ia.urec = st.urec_item[k];
    ia.n_uniq = &st.hdr->n_uniq[k][0]; ia.hot_n = &st.hdr->n_hot[k]; ia.hot_list = st.hot_list[k];
    ia.item_cate = item_cate; ia.cnt_uc = st.cnt_uc[k];
    ia.nfin = (ia.nb + 15) / 16;
    hipLaunchKernelGGL(k_isort_hist, dim3(ia.nbu + ia.nblk), dim3(1024), 0, hs, ia, ca);
    CHECK_LAUNCH("k_isort_hist");
    hipLaunchKernelGGL(k_isort_scatter, dim3(ia.nblk), dim3(1024), 0, hs, ia);
    CHECK_LAUNCH("k_isort_scatter");
    UsortArgs ua;   // (the user side's sort rides in this launch: as long as a bucket block, and needed by nothing before the step)
    memset(&ua, 0, sizeof(ua));
    if (usort) {
      ua.u = b->u; ua.B = b->B; ua.U = d->user_count;
      ua.cur = st.cur_user[k]; ua.off = st.off_user[k]; ua.urec = st.urec_user[k]; ua.n_uniq = &st.hdr->n_uniq[k][1];
    }
    hipLaunchKernelGGL(k_isort_bucket, dim3(ia.nb + (usort ? 1 : 0)), dim3(1024), 0, hs, ia, ua);
    CHECK_LAUNCH("k_isort_bucket");
  } else {
    hipLaunchKernelGGL(k_count, dim3((b->B + 255) / 256 + (nthr + 255) / 256), dim3(256), 0, hs, ca);
    CHECK_LAUNCH("k_count");
  }
  sa.cnt[0] = st.cnt_item[k]; sa.cnt[1] = st.cnt_uc[k]; sa.cnt[2] = st.cnt_user[k];
  sa.off[0] = st.off_item[k]; sa.off[1] = st.off_uc[k]; sa.off[2] = st.off_user[k];
  sa.cur[0] = st.cur_item[k]; sa.cur[1] = st.cur_uc[k]; sa.cur[2] = st.cur_user[k];
  scanned_rows(d, ix, sa.n);
  sa.blk0[0] = 0;
  sa.blk0[1] = (sa.n[0] + 4095) / 4096;
  sa.blk0[2] = sa.blk0[1] + (sa.n[1] + 4095) / 4096;
  if (usort) {
    if (!isort) {   // (with the items sorted as well, k_isort_bucket's launch had it)
      sa.us.u = b->u; sa.us.B = b->B; sa.us.U = d->user_count;
      sa.us.cur = st.cur_user[k]; sa.us.off = st.off_user[k]; sa.us.urec = st.urec_user[k]; sa.us.n_uniq = &st.hdr->n_uniq[k][1];
    }
  }
  const int nscan = sa.blk0[2] + (sa.n[2] + 4095) / 4096;
  sa.urec[0] = st.urec_item[k]; sa.urec[2] = st.urec_user[k];
  sa.hot_n[0] = &st.hdr->n_hot[k]; sa.hot_list[0] = st.hot_list[k];
  sa.total[0] = sa.total[1] = sa.total[2] = 1;
  sa.flag[2] = st.flag_user[k];
  // (sa.bs_ticket = st.scan_ticket + k: the sums scanned by the last block of k_scan_block_sums, one prefix read per scan
  //  block -- measured slower: 3663 publishing atomics on consecutive words, 134 -> 162 us/step at 10 M / 5 M rows)
  sa.sparse = ix.sparse;
  sa.n_uniq[0] = &st.hdr->n_uniq[k][0]; sa.n_uniq[1] = nullptr; sa.n_uniq[2] = &st.hdr->n_uniq[k][1];
  if (ix.rank) {   // (a ranking block only for a launch that will read it: plan_front)
    sa.bal.sl = b->sl; sa.bal.sl_new = b->sl_new;
    sa.bal.B = b->B; sa.bal.Ls = d->Ls; sa.bal.Sn = b->Sn;
    sa.bal.by_window = ix.by_window;
    sa.bal.perm = st.perm[k];
  }
  if ((rc = launch_scan(sa, nscan, st.scan_bsum[k], hs))) return rc;
  if (ix.uc_list) {
    hipLaunchKernelGGL(k_uc_fill, dim3((b->B + 255) / 256), dim3(256), 0, hs, b->u_cate, b->B, d->cate_count, st.cur_uc[k], st.uc_list[k]);
    CHECK_LAUNCH("k_uc_fill");
  }
  return TLSAN_OK;
}

// shared front half of train_step / grads, as planned (plan_front): index build, fused fwd+bwd, dK partials; fills f but
// for plan_tail's fields
static int run_backward(const tlsan_dims* d, const Shape& s, const tlsan_params* p, const tlsan_batch* b,
                        const tlsan_hparams* hp, const tlsan_step_out* out, const Ws& w, const St& st,
                        const tlsan_dense_layout& L, hipStream_t hs, const FrontPlan& fp, FinArgs* f, bool two = false) {
  const int k = hp->index_slot;
  int rc;
  prof_mark(0, hs);
  if (!hp->index_prebuilt && (rc = build_index(d, b, fp.ix, p->item_cate, st, k, hs))) return rc;
  // --- fused forward + backward
  FwdArgs a;
  fill_fwd(a, d, p, b, fp, L);
  a.logits_i = (out && out->logits) ? out->logits : w.logits;
  if (out && out->started) { a.started = out->started; a.started_val = out->started_value; }
  a.Gi = w.Gi; a.Gb = w.Gb; a.Gu = w.Gu; a.Gc = w.Gc; a.WU = w.WU;
  a.cur_item = st.cur_item[k]; a.cur_user = st.cur_user[k]; a.cur_uc = st.cur_uc[k];
  a.uc_by_sample = fp.ix.uc_list ? 1 : 0;
  a.cseg = fp.ix.cseg ? 1 : 0;
  a.perm = fp.read_rank ? st.perm[k] : nullptr;
  if (two) { a.fix_hdr = st.hdr; a.fix_args = st.fix_args; }   // (the two-launch form: the snapshot, and a clipped predecessor's correction)
  a.gLong = w.gLong; a.gDB = w.gDB; a.gStat = w.gStat; a.partials = w.partials; a.Kp = w.Kp;
  if (hp->dropout != 0.0f) {
    if (!(hp->dropout > 0.0f && hp->dropout < 1.0f)) return fail(TLSAN_E_BADARG, "dropout must be in [0, 1)");
    const float keep = (float)(1.0 - (double)hp->dropout);
    const double t = (double)keep * 4294967296.0;
    a.drop_thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    a.drop_inv = 1.0f / keep;
    a.drop_seed = hp->dropout_seed;
    a.drop_sample0 = hp->dropout_sample0;
  }
  prof_mark(1, hs);
  if ((rc = launch_fwd(s, true, fp, a, hs))) return rc;
  prof_mark(2, hs);
  // --- dense-parameter gradients (fused: the dK partials were left by k_fwd_bwd, one per workgroup)
  if (!fp.fuse_dk) {
    const int spw = dk_spw(b->B, s.D), nq = (s.D / 64) * (s.D / 64);
    const dim3 grid(nq * fp.nsplit), blk(DK_WAVES * 64);
#define DK_LAUNCH(DD)                                                                                           \
  do {                                                                                                          \
    (void)hipFuncSetAttribute((const void*)k_dk_partial<DD>, hipFuncAttributeMaxDynamicSharedMemorySize, DK_SMEM_BYTES); \
    hipLaunchKernelGGL(k_dk_partial<DD>, grid, blk, DK_SMEM_BYTES, hs, w.gLong, w.gDB, b->B, spw, w.Kp);        \
  } while (0)
    if (s.D == 64) DK_LAUNCH(64);
    else if (s.D == 128) DK_LAUNCH(128);
    else DK_LAUNCH(256);
#undef DK_LAUNCH
  }
  CHECK_LAUNCH("k_dk_partial");
  prof_mark(3, hs);
  f->lay = L; f->partials = w.partials; f->nrec = fp.ngroups; f->Kp = w.Kp; f->nsplit = fp.nsplit;
  f->sqd = w.sqd; f->scal = w.scal;
  f->S_delta = st.S_delta; f->delta_nrec = st.nrec; f->S_total = st.S_total;
  f->hdr = st.hdr; f->lr = hp->lr; f->reg = hp->reg; f->clip = hp->clip; f->inv_B = 1.0f / (float)b->B;
  f->norm_mode = hp->norm_mode;
  f->out_loss = out ? out->loss : nullptr;
  f->out_gnorm = out ? out->gnorm : nullptr;
  f->out_sq = out ? out->sq_rows : nullptr;
  return TLSAN_OK;
}

static int prep_step(const tlsan_dims* d, Shape* s, const tlsan_params* p, const tlsan_batch* b, const tlsan_hparams* hp,
                     void* state, void* ws, size_t ws_bytes, Ws* w, St* st) {
  int rc = shape_of(d, s);
  if (rc) return rc;
  if ((rc = check_params(p))) return rc;
  if ((rc = check_batch(d, b, true))) return rc;
  if (!hp) return fail(TLSAN_E_BADARG, "hparams is NULL");
  if (hp->l2_mode != TLSAN_L2_DENSE && hp->l2_mode != TLSAN_L2_LAZY) return fail(TLSAN_E_BADARG, "l2_mode");
  if (hp->index_slot < 0 || hp->index_slot >= TLSAN_INDEX_SLOTS) return fail(TLSAN_E_BADARG, "index_slot must be 0 .. %d", TLSAN_INDEX_SLOTS - 1);
  if (hp->l2_mode == TLSAN_L2_LAZY) {
    if (hp->norm_mode != TLSAN_NORM_TF18) return fail(TLSAN_E_UNSUPPORTED, "TLSAN_L2_LAZY supports norm_mode TF18 only");
    if (p->scale != tlsan_state_scale(state)) return fail(TLSAN_E_BADARG, "TLSAN_L2_LAZY needs params->scale == tlsan_state_scale(state)");
  }
  if (hp->norm_mode != TLSAN_NORM_TF18 && hp->norm_mode != TLSAN_NORM_DEDUP) return fail(TLSAN_E_BADARG, "norm_mode");
  if (!state || !ws) return fail(TLSAN_E_WORKSPACE, "state / ws is NULL");
  carve(d, *s, b->B, b->Sn, (char*)ws, w);
  if (w->bytes > ws_bytes) return fail(TLSAN_E_WORKSPACE, "workspace too small: need %zu have %zu", w->bytes, ws_bytes);
  carve_state(d, *s, (char*)state, st);
  return TLSAN_OK;
}

// dedup-norm mode: per-row squared norms of the SUMMED gradients (ROWNORM pass), then the coefficient
static int clip_dedup(const ApplyArgs& A, const tlsan_hparams* hp, const tlsan_step_out* out, const Ws& w,
                      const St& st, hipStream_t hs) {
  ApplyArgs R = A;
  R.part_out = w.rownorm_part;
  int rc = launch_apply(AP_ROWNORM, R, false, hs);
  if (rc) return rc;
  hipLaunchKernelGGL(k_clip_dedup, dim3(1), dim3(256), 0, hs, w.rownorm_part, st.nbI + st.nbU + st.nbC, w.sqd, w.nfin,
                     st.hdr, hp->clip, out ? out->gnorm : nullptr);
  CHECK_LAUNCH("k_clip_dedup");
  return TLSAN_OK;
}

// the plan's launches: the finalize (run_backward filled the front half of its arguments), then the second launch
static int launch_tail(const Shape& s, const TailPlan& P, const tlsan_hparams* hp, const tlsan_step_out* out, const Ws& w,
                       const St& st, hipStream_t hs) {
  static const char* const fin_name[] = {"k_dense_finalize", "k_finalize_presum", "k_finalize_update"};
  const ApplyArgs& A = P.fin.A;
  const bool bf16 = A.p.table_dtype == TLSAN_TABLE_BF16;
  const dim3 blk(256);
  int rc;
  pair_of(s.D, s.DH)->finalize(P.fin, hs);   // the dense finalize of the shape's pair
  CHECK_LAUNCH(fin_name[P.fin.kind]);
  prof_mark(4, hs);
  switch (P.form) {
    case TAIL_APPLY:
      if (hp->norm_mode == TLSAN_NORM_DEDUP && (rc = clip_dedup(A, hp, out, w, st, hs))) return rc;
      if ((rc = launch_apply(P.update ? AP_UPDATE : AP_GRADS, A, true, hs))) return rc;
      break;
    case TAIL_SPLIT:
      if (P.update && (A.opt == TLSAN_OPT_ADAGRAD || A.opt == TLSAN_OPT_ROWWISE_ADAGRAD)) {   // lazy (row-wise) Adagrad: one accumulator
#define ADAGRAD_LAUNCH(RW)                                                                                                      \
  do {                                                                                                                          \
    if (bf16 && P.wide) hipLaunchKernelGGL((k_update_lazy_adagrad<true, TLSAN_TABLE_BF16, RW>), P.grid, blk, 0, hs, A, P.nbC16);  \
    else if (bf16) hipLaunchKernelGGL((k_update_lazy_adagrad<false, TLSAN_TABLE_BF16, RW>), P.grid, blk, 0, hs, A, P.nbC16);      \
    else if (P.wide) hipLaunchKernelGGL((k_update_lazy_adagrad<true, TLSAN_TABLE_F32, RW>), P.grid, blk, 0, hs, A, P.nbC16);      \
    else hipLaunchKernelGGL((k_update_lazy_adagrad<false, TLSAN_TABLE_F32, RW>), P.grid, blk, 0, hs, A, P.nbC16);                 \
  } while (0)
        if (A.opt == TLSAN_OPT_ROWWISE_ADAGRAD) ADAGRAD_LAUNCH(true);
        else ADAGRAD_LAUNCH(false);
#undef ADAGRAD_LAUNCH
        CHECK_LAUNCH("k_update_lazy_adagrad");
      } else if (P.update && A.opt != TLSAN_OPT_SGD) {   // lazy Adam / RMSProp / Adadelta: the used rows and their slots
        if (bf16 && P.wide) hipLaunchKernelGGL((k_update_lazy_opt<true, TLSAN_TABLE_BF16>), P.grid, blk, 0, hs, A, P.nbC16);
        else if (bf16) hipLaunchKernelGGL((k_update_lazy_opt<false, TLSAN_TABLE_BF16>), P.grid, blk, 0, hs, A, P.nbC16);
        else if (P.wide) hipLaunchKernelGGL((k_update_lazy_opt<true, TLSAN_TABLE_F32>), P.grid, blk, 0, hs, A, P.nbC16);
        else hipLaunchKernelGGL((k_update_lazy_opt<false, TLSAN_TABLE_F32>), P.grid, blk, 0, hs, A, P.nbC16);
        CHECK_LAUNCH("k_update_lazy_opt");
      } else if (P.update) {   // the short elementwise update of the summed rows
        if (bf16 && P.wide) hipLaunchKernelGGL((k_update_lazy<true, TLSAN_TABLE_BF16>), P.grid, blk, 0, hs, A, P.nbC16);
        else if (bf16) hipLaunchKernelGGL((k_update_lazy<false, TLSAN_TABLE_BF16>), P.grid, blk, 0, hs, A, P.nbC16);
        else if (P.wide) hipLaunchKernelGGL((k_update_lazy<true, TLSAN_TABLE_F32>), P.grid, blk, 0, hs, A, P.nbC16);
        else hipLaunchKernelGGL((k_update_lazy<false, TLSAN_TABLE_F32>), P.grid, blk, 0, hs, A, P.nbC16);
        CHECK_LAUNCH("k_update_lazy");
      } else if (A.csplit > 1) {   // the split workgroups left exact double sums: round them into the output
        hipLaunchKernelGGL(k_rc64_to_float, P.grid, blk, 0, hs, A.Rc64, A.Rc, A.C * A.dc);
        CHECK_LAUNCH("k_rc64_to_float");
      }
      break;
    case TAIL_SPEC_SHARED:
    case TAIL_SPEC:
      if (P.two) break;   // (nothing follows the finalize: its workgroups committed, TailPlan::two)
      tlsan_launch_spec_commit(P.wide, bf16, P.form == TAIL_SPEC_SHARED, P.grid, A, hs);
      CHECK_LAUNCH("k_spec_commit");
      break;
  }
  prof_mark(5, hs);
  prof_step_done();
  return TLSAN_OK;
}

int tlsan_batch_pack(const tlsan_packed* set, const int32_t* order, int32_t lo, const tlsan_batch* out, int32_t Ls,
                     int32_t is_test, void* stream) {
  if (!set || !order || !out) return fail(TLSAN_E_BADARG, "tlsan_batch_pack: NULL argument");
  if (!set->u || !set->cate || !set->hist_off || !set->sess_off || !set->target || !set->second)
    return fail(TLSAN_E_BADARG, "tlsan_batch_pack: NULL pointer in the packed set");
  if (out->B < 1 || out->Sn < 0 || Ls < 1 || lo < 0 || lo + out->B > set->n)
    return fail(TLSAN_E_BADARG, "tlsan_batch_pack: samples [%d, %d) outside the set of %d", lo, lo + out->B, set->n);
  if (!out->u || !out->i || !out->hist_i || !out->hist_t || !out->sl || !out->sl_new || !out->u_cate ||
      (out->Sn > 0 && !out->hist_i_new) || (is_test ? !out->j : !out->y))
    return fail(TLSAN_E_BADARG, "tlsan_batch_pack: NULL output array");
  if ((size_t)out->B * (Ls + out->Sn + 1) >= ((size_t)1 << 31)) return fail(TLSAN_E_UNSUPPORTED, "B*S overflows int32");
  PackArgs a;
  a.set = *set; a.order = order; a.lo = lo; a.Ls = Ls; a.is_test = is_test ? 1 : 0; a.out = *out;
  const int nthr = out->B * (Ls + out->Sn + 1);
  hipLaunchKernelGGL(k_batch_pack, dim3((nthr + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
  CHECK_LAUNCH("k_batch_pack");
  return TLSAN_OK;
}

int tlsan_batch_index(const tlsan_dims* d, const tlsan_batch* b, const int32_t* item_cate, void* state, int32_t slot, void* stream) {
  Shape s; St st;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if ((rc = check_batch(d, b, true))) return rc;
  const bool lazy_sgd = (slot & TLSAN_INDEX_FOR_LAZY_SGD) != 0;
  slot &= ~TLSAN_INDEX_FOR_LAZY_SGD;
  if (slot < 0 || slot >= TLSAN_INDEX_SLOTS) return fail(TLSAN_E_BADARG, "index slot must be 0 .. %d", TLSAN_INDEX_SLOTS - 1);
  if (!state) return fail(TLSAN_E_WORKSPACE, "state is NULL");
  carve_state(d, s, (char*)state, &st);
  return build_index(d, b, plan_index(d, s, b, lazy_sgd), item_cate, st, slot, (hipStream_t)stream);
}

// (for tests and tools: where an index slot lives in the state -- carve_state's own answers, as offsets from a null base)
int tlsan_index_layout_of(const tlsan_dims* d, int32_t slot, tlsan_index_layout* out) {
  Shape s; St st;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if (!out) return fail(TLSAN_E_BADARG, "tlsan_index_layout_of: out is NULL");
  if (slot < 0 || slot >= TLSAN_INDEX_SLOTS) return fail(TLSAN_E_BADARG, "index slot must be 0 .. %d", TLSAN_INDEX_SLOTS - 1);
  carve_state(d, s, nullptr, &st);
  auto at = [](const void* p) { return (int64_t)(uintptr_t)p; };
  const Capacity cap = plan_capacity(d, s, 1);
  memset(out, 0, sizeof(*out));
  out->cnt_item = at(st.cnt_item[slot]); out->cnt_uc = at(st.cnt_uc[slot]); out->cnt_user = at(st.cnt_user[slot]);
  out->off_item = at(st.off_item[slot]); out->off_uc = at(st.off_uc[slot]); out->off_user = at(st.off_user[slot]);
  out->cur_item = at(st.cur_item[slot]); out->cur_uc = at(st.cur_uc[slot]); out->cur_user = at(st.cur_user[slot]);
  out->urec_item = at(st.urec_item[slot]); out->urec_user = at(st.urec_user[slot]);
  out->perm = at(st.perm[slot]); out->uc_list = at(st.uc_list[slot]); out->hot_list = at(st.hot_list[slot]);
  out->flag_user = at(st.flag_user[slot]);
  out->scan_ticket = at(st.scan_ticket);
  out->n_uniq = at(st.hdr) + (int64_t)(offsetof(StateHdr, n_uniq) + sizeof(int32_t) * 2 * slot);
  out->n_hot = at(st.hdr) + (int64_t)(offsetof(StateHdr, n_hot) + sizeof(int32_t) * slot);
  out->rank_cap = cap.rank_cap; out->uc_list_cap = cap.uc_list_cap;
  out->ap_hot = AP_HOT; out->ap_hot_cap = AP_HOT_CAP;
  return TLSAN_OK;
}

// (for tests and tools: what plan_index decides for a batch of B samples with Sn session columns -- host fields only)
int tlsan_index_plan_of(const tlsan_dims* d, int32_t B, int32_t Sn, int32_t flags, tlsan_index_plan* out) {
  Shape s;
  int rc = shape_of(d, &s);
  if (rc) return rc;
  if (!out || B < 1 || Sn < 0) return fail(TLSAN_E_BADARG, "tlsan_index_plan_of: bad arguments (B=%d, Sn=%d)", B, Sn);
  if (flags & ~TLSAN_INDEX_FOR_LAZY_SGD) return fail(TLSAN_E_BADARG, "tlsan_index_plan_of: flags must be 0 or TLSAN_INDEX_FOR_LAZY_SGD");
  tlsan_batch b;
  memset(&b, 0, sizeof(b));
  b.B = B; b.Sn = Sn;
  const IndexPlan ix = plan_index(d, s, &b, (flags & TLSAN_INDEX_FOR_LAZY_SGD) != 0);
  int32_t n[3];
  scanned_rows(d, ix, n);
  memset(out, 0, sizeof(*out));
  out->cseg = ix.cseg; out->uc_list = ix.uc_list; out->usort = ix.usort; out->isort = ix.isort;
  out->sparse = ix.sparse; out->rank = ix.rank; out->by_window = ix.by_window;
  out->two_level = scan_two_level(n) ? 1 : 0;
  return TLSAN_OK;
}

// (rows: the four tables of the set are [rows] floats -- TLSAN_OPT_ROWWISE_ADAGRAD -- whose strides are not looked at)
static int check_slot(const tlsan_params* q, const char* name, bool rows = false) {
  if (!q || !q->item_emb || !q->item_b || !q->user_emb || !q->usert_emb || !q->cate_emb || !q->dense)
    return fail(TLSAN_E_BADARG, "tlsan_optimizer: NULL table in %s", name);
  if (!rows && (q->ld_item % 4 || q->ld_user % 4)) return fail(TLSAN_E_UNSUPPORTED, "tlsan_optimizer: row strides of %s must be multiples of 4 floats", name);
  return TLSAN_OK;
}

int tlsan_train_step(const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, const tlsan_hparams* hp,
                     const tlsan_step_out* out, void* state, void* ws, size_t ws_bytes, void* stream) {
  return tlsan_train_step_opt(d, p, b, hp, nullptr, out, state, ws, ws_bytes, stream);
}

int tlsan_train_step_opt(const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, const tlsan_hparams* hp,
                         const tlsan_optimizer* opt, const tlsan_step_out* out, void* state, void* ws, size_t ws_bytes,
                         void* stream) {
  Shape s; Ws w; St st;
  int rc = prep_step(d, &s, p, b, hp, state, ws, ws_bytes, &w, &st);
  if (rc) return rc;
  const bool other = opt && opt->kind != TLSAN_OPT_SGD;
  const int kind = other ? opt->kind & ~TLSAN_OPT_LAZY : TLSAN_OPT_SGD;
  const bool adagrad = kind == TLSAN_OPT_ADAGRAD || kind == TLSAN_OPT_ROWWISE_ADAGRAD;
  if (other) {
    if (kind != TLSAN_OPT_ADAM && kind != TLSAN_OPT_RMSPROP && kind != TLSAN_OPT_ADADELTA && !adagrad)
      return fail(TLSAN_E_BADARG, "tlsan_optimizer: kind %d (TLSAN_OPT_LAZY goes with ADAM, RMSPROP, ADADELTA, ADAGRAD or ROWWISE_ADAGRAD)", opt->kind);
    if (adagrad && !(opt->kind & TLSAN_OPT_LAZY))
      return fail(TLSAN_E_UNSUPPORTED, "tlsan_optimizer: kind %d: the dense sweep is not built for ADAGRAD / ROWWISE_ADAGRAD (OR TLSAN_OPT_LAZY in)", opt->kind);
    if (opt->kind & TLSAN_OPT_LAZY) {   // (prep_step checked the rest of the lazy-L2 contract: TF18 norm, params->scale)
      if (hp->l2_mode != TLSAN_L2_LAZY) return fail(TLSAN_E_UNSUPPORTED, "TLSAN_OPT_LAZY updates the used rows only: l2_mode must be TLSAN_L2_LAZY");
    } else if (hp->l2_mode != TLSAN_L2_DENSE) {
      return fail(TLSAN_E_UNSUPPORTED, "optimizers other than sgd update every row: l2_mode must be TLSAN_L2_DENSE");
    }
    // (Adagrad keeps one accumulator: slot2 is never looked at)
    if ((rc = check_slot(opt->slot1, "slot1", kind == TLSAN_OPT_ROWWISE_ADAGRAD)) || (!adagrad && (rc = check_slot(opt->slot2, "slot2")))) return rc;
    if (kind == TLSAN_OPT_ADAM && opt->step < 1) return fail(TLSAN_E_BADARG, "tlsan_optimizer: Adam's step counts from 1");
  }
  hipStream_t hs = (hipStream_t)stream;
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  const FrontPlan fp = plan_front(d, s, b, hp, plan_sparse(hp, true, 0));
  ApplyArgs A;
  fill_apply(A, d, s, p, &fp.ix, hp, w, st, L);
  if (other) {
    A.opt = kind;
    A.s1 = norm_params(opt->slot1, d);
    if (!adagrad) A.s2 = norm_params(opt->slot2, d);
    A.ob1 = opt->beta1; A.ob2 = opt->beta2; A.oeps = opt->epsilon;
    if (kind == TLSAN_OPT_ADAM) A.oalpha = adam_alpha(hp->lr, opt->beta1, opt->beta2, opt->step);
  }
  TailPlan P;
  if ((rc = plan_tail(d, s, b, hp, w, A, true, &P))) return rc;
  // (a correction the state may owe: at the head of this step's fused kernel, or a flush in front of the step)
  if ((rc = step_flush(d, p, state, st, hs, P.two, hp->index_prebuilt != 0))) return rc;
  if ((rc = run_backward(d, s, p, b, hp, out, w, st, L, hs, fp, &P.fin.f, P.two))) return rc;
  if (P.two) two_list(state);
  return launch_tail(s, P, hp, out, w, st, hs);
}

int tlsan_grads(const tlsan_dims* d, const tlsan_params* p, const tlsan_batch* b, const tlsan_hparams* hp,
                const tlsan_grads_out* g, const tlsan_step_out* out, void* state, void* ws, size_t ws_bytes, void* stream) {
  Shape s; Ws w; St st;
  int rc = prep_step(d, &s, p, b, hp, state, ws, ws_bytes, &w, &st);
  if (rc) return rc;
  if (!g || !g->item_emb || !g->item_b || !g->user_emb || !g->usert_emb || !g->cate_emb || !g->dense)
    return fail(TLSAN_E_BADARG, "NULL gradient output");
  hipStream_t hs = (hipStream_t)stream;
  tlsan_dense_layout L;
  tlsan_dense_layout_of(d, &L);
  const FrontPlan fp = plan_front(d, s, b, hp, plan_sparse(hp, false, g->sparse));
  ApplyArgs A;
  fill_apply(A, d, s, p, &fp.ix, hp, w, st, L);
  A.go = *g;
  if (A.go.ld_item == 0) A.go.ld_item = d->d_item;
  if (A.go.ld_itemb == 0) A.go.ld_itemb = 1;
  if (A.go.ld_user == 0) A.go.ld_user = d->d_item;
  if (A.go.ld_usert == 0) A.go.ld_usert = d->Ls;
  if (A.go.ld_item % 4 || A.go.ld_user % 4) return fail(TLSAN_E_UNSUPPORTED, "gradient row strides must be multiples of 4 floats");
  TailPlan P;
  if ((rc = plan_tail(d, s, b, hp, w, A, false, &P))) return rc;
  if ((rc = flush_if_listed(d, p, state, st, hs))) return rc;
  if ((rc = run_backward(d, s, p, b, hp, out, w, st, L, hs, fp, &P.fin.f))) return rc;
  return launch_tail(s, P, hp, out, w, st, hs);
}

int tlsan_debug_stamps(void* device_buf) {
  g_stamps = (unsigned long long*)device_buf;
  return TLSAN_OK;
}

int tlsan_profile_stride(int every) {
  if (every < 1) return fail(TLSAN_E_BADARG, "profile stride must be >= 1");
  g_prof_stride = every;
  return TLSAN_OK;
}

int tlsan_profile_enable(int level) {
  if (level < 0 || level > 2) return fail(TLSAN_E_BADARG, "profile level must be 0..2");
  if (level > 0 && !g_prof_ev) {
    g_prof_ev = (hipEvent_t*)malloc(sizeof(hipEvent_t) * PROF_MAX_STEPS * PROF_MARKS);
    if (!g_prof_ev) return fail(TLSAN_E_WORKSPACE, "out of host memory");
    for (int k = 0; k < PROF_MAX_STEPS * PROF_MARKS; ++k)
      if (hipEventCreate(&g_prof_ev[k]) != hipSuccess) return fail(TLSAN_E_LAUNCH, "hipEventCreate");
  }
  g_prof_level = level;
  g_prof_n = 0;
  g_prof_tick = 0;
  return TLSAN_OK;
}

int tlsan_profile_collect(float* host_ms, int max_steps) {
  if (!host_ms || max_steps < 0) return fail(TLSAN_E_BADARG, "bad profile buffer");
  int n = g_prof_n < max_steps ? g_prof_n : max_steps;
  for (int k = 0; k < n; ++k) {
    hipEvent_t* e = g_prof_ev + (size_t)k * PROF_MARKS;
    for (int sgm = 0; sgm < TLSAN_PROF_SEGMENTS; ++sgm) {
      float ms = 0.0f;
      if (g_prof_level == 2 || sgm == 1) {
        if (hipEventSynchronize(e[sgm + 1]) != hipSuccess || hipEventElapsedTime(&ms, e[sgm], e[sgm + 1]) != hipSuccess)
          return fail(TLSAN_E_LAUNCH, "hipEventElapsedTime");
      }
      host_ms[k * TLSAN_PROF_SEGMENTS + sgm] = ms;
    }
  }
  g_prof_n = 0;
  return n;
}

}  // extern "C"

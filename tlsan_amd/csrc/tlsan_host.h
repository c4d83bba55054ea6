// tlsan_host.h -- what the host units of the C ABI share (tlsan_api.hip: core, training and state; tlsan_api_plan.hip: the
// plans of a training step; tlsan_api_eval.hip: evaluation; tlsan_api_shard.hip: rows and the sharded step): error reporting,
// the shape and workspace carve-up, the launchers of the kernel units, and the few host helpers one unit offers another.  Everything here is internal to the
// library (hidden visibility: none of it is an exported symbol).
#pragma once
#include <stdlib.h>
#include <string.h>

#include "tlsan_common.h"

struct ScanArgs;                                   // tlsan_index_args.h
struct FinLaunch; struct ApplyArgs;                // tlsan_update_args.h
struct TopkArgs;                                   // tlsan_topk.h
struct CandArgs; struct NegArgs; struct ExclArgs;  // tlsan_cand.h
struct EvalArgs;                                   // tlsan_eval.h
struct SimArgs; struct VecArgs;                    // tlsan_similar.h
struct ScopeArgs; struct ScopedTopkArgs; struct ScopedSimArgs;   // tlsan_scope.h
struct ListsArgs;                                  // tlsan_lists.h

#pragma GCC visibility push(hidden)

// the calling thread's message behind tlsan_last_error(): ONE thread_local object, defined in tlsan_api.hip
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define CHECK_LAUNCH(what)                                                         \
  do {                                                                             \
    hipError_t e_ = hipGetLastError();                                             \
    if (e_ != hipSuccess) return fail(TLSAN_E_LAUNCH, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

static inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct Shape {  // derived geometry of the supported (d, heads) combinations
  int D, DH, NSB, NPB, CW;
  int SG;   // samples per pass of the pair's small-group training kernel, 0: it has none (Pair, tlsan_api.hip)
};
int shape_of(const tlsan_dims* d, Shape* s);
int check_params(const tlsan_params* p);

// fill in the default (dense) row strides
static inline tlsan_params norm_params(const tlsan_params* p, const tlsan_dims* d) {
  tlsan_params q = *p;
  if (q.ld_item == 0) q.ld_item = d->d_item;
  if (q.ld_itemb == 0) q.ld_itemb = 1;
  if (q.ld_user == 0) q.ld_user = d->d_item;
  if (q.ld_usert == 0) q.ld_usert = d->Ls;
  return q;
}

// Adam's step size (adam.py): lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
static inline float adam_alpha(float lr, float beta1, float beta2, int step) {
  return (float)((double)lr * sqrt(1.0 - pow((double)beta2, step)) / (1.0 - pow((double)beta1, step)));
}

#define EVAL_DENSE_MAX ((size_t)256 << 20)  // all-items scoring materialises all_emb (model.py:89-90) up to this size
struct Ws {  // carve-up of the caller's scratch buffer
  float *Rc, *Ri, *Rb, *Ru;  // summed rows of the split lazy update
  float *Gi, *Gb, *Gu, *Gc, *gLong, *gDB, *gStat, *partials, *Kp, *gd, *sqd, *scal, *logits, *s_label;
  float* all_emb;  // evaluation: dense [I, D] item matrix (NULL when it would exceed EVAL_DENSE_MAX bytes)
  double* rownorm_part;
  double* rownorm;
  size_t bytes;
  int nfin, nbK, nbS, WU;
};
void carve(const tlsan_dims* d, const Shape& s, int B, int Sn, char* base, Ws* w);

// ---- the fused kernel's units (tlsan_attn_d*.hip)
struct LaunchEvents { hipEvent_t start, stop; };   // optional time stamps of the dispatch (tlsan_attn_inst.h)
hipError_t tlsan_launch_fwd_bwd_d64(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
hipError_t tlsan_launch_fwd_bwd_d128(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
hipError_t tlsan_launch_fwd_bwd_d256(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
hipError_t tlsan_launch_fwd_bwd_d128w4(const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);   // training, 8-sample workgroups
hipError_t tlsan_launch_fwd_bwd_d64h4(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
hipError_t tlsan_launch_fwd_bwd_d128h16(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
hipError_t tlsan_launch_fwd_bwd_d128h4(bool train, bool lstream, const FwdArgs& a, int grid, hipStream_t st, LaunchEvents ev);
// ---- the dense finalize of every (d, heads) pair (tlsan_update_d*.hip)
void tlsan_launch_finalize_d64(const FinLaunch& L, hipStream_t hs);
void tlsan_launch_finalize_d64h4(const FinLaunch& L, hipStream_t hs);
void tlsan_launch_finalize_d128(const FinLaunch& L, hipStream_t hs);
void tlsan_launch_finalize_d128h16(const FinLaunch& L, hipStream_t hs);
void tlsan_launch_finalize_d128h4(const FinLaunch& L, hipStream_t hs);
void tlsan_launch_finalize_d256(const FinLaunch& L, hipStream_t hs);
// k_spec_commit of every pair (compiled beside k_finalize_update: tlsan_update_d128.hip)
void tlsan_launch_spec_commit(bool wide, bool bf16, bool shared, dim3 grid, const ApplyArgs& A, hipStream_t hs);
// ... and k_spec_flush: the correction a clipped two-launch step owes, from the arguments it left in the state
void tlsan_launch_spec_flush(bool wide, bool bf16, const void* args, void* hdr, hipStream_t hs);
// ---- top-K selection over all items (tlsan_topk.hip)
hipError_t tlsan_launch_topk(const TopkArgs& a, int D, int nslices, hipStream_t hs);
hipError_t tlsan_launch_topk_merge(const int32_t* cid, const float* csc, int B, int nl, int K, int32_t* ids, float* scores,
                                   hipStream_t hs);
// ---- similar-items lists (tlsan_similar.hip): the inv pass (with the dense item matrix), the selection, the query vectors
hipError_t tlsan_launch_sim_prep(const EvalArgs& e, int D, float* inv, hipStream_t hs);
hipError_t tlsan_launch_similar_topk(const SimArgs& a, int D, int nslices, hipStream_t hs);
hipError_t tlsan_launch_item_vectors(const VecArgs& a, int D, hipStream_t hs);
// ---- scoped lists (tlsan_scope.hip): the selections over a subset of the items, the inv pass of the subset (count >= 1)
hipError_t tlsan_launch_scoped_topk(const ScopedTopkArgs& a, int D, int nslices, hipStream_t hs);
hipError_t tlsan_launch_scoped_similar(const ScopedSimArgs& a, int D, int nslices, hipStream_t hs);
hipError_t tlsan_launch_scope_inv(const EvalArgs& e, const ScopeArgs& s, int count, int D, float* inv, hipStream_t hs);
// ---- indexed lists (tlsan_lists.hip): the grouping of the valid (row, probe) pairs by list, in the caller's workspace
hipError_t tlsan_launch_lists_group(const ListsArgs& l, hipStream_t hs);
// ---- candidate scoring, candidate ranks, negative sampling (tlsan_cand.hip)
hipError_t tlsan_launch_score_cand(const CandArgs& a, int D, hipStream_t hs);
hipError_t tlsan_launch_cand_ranks(const int32_t* cand, const float* scores, int B, int C, int32_t* ranks, hipStream_t hs);
hipError_t tlsan_launch_sample_neg(const NegArgs& a, hipStream_t hs);
hipError_t tlsan_launch_excl_ahead(const ExclArgs& a, int D, hipStream_t hs);

// ---- tlsan_api.hip owns the index scan (tlsan_index.h) and k_reduce_double
int launch_scan(ScanArgs& sa, int nscan, long long* bsum, hipStream_t hs);
int scan_compact_impl(const int32_t* cnt, int32_t n, int32_t* prefix, int32_t* uniq, int32_t* n_uniq, long long* bsum,
                      hipStream_t hs);
int launch_reduce_double(const double* v, int n, double* out, hipStream_t hs);
// ---- tlsan_api_shard.hip owns the generic index kernels (tlsan_rows.h)
// static CSR category -> items from item_cate (a counting sort): cnt / cur [C], off [C], items [I]
int build_cate_csr(const int32_t* item_cate, int I, int C, int32_t* cnt, int32_t* off, int32_t* cur, int32_t* items,
                   hipStream_t hs);

#pragma GCC visibility pop

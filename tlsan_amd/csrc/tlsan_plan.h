// tlsan_plan.h -- the plans of a training step, between the unit that makes them (tlsan_api_plan.hip) and the unit that
// issues them (tlsan_api.hip): the front (the destination index, the fused kernel's launch, the dK product) and the tail
// (everything after the fused kernel).  The rules behind the plans are static functions of the planning unit: no other
// unit can ask them again.
#pragma once
#include "tlsan_host.h"
#include "tlsan_update_args.h"

// What build_index builds for a batch.  Planned from the dims, the shape, the batch and the sparse flag only -- what
// tlsan_batch_index has, one or two steps ahead of the step and without its hyper-parameters (plan_index).
struct IndexPlan {
  bool cseg;        // category segments: item uses are counted per category (CountArgs.cseg, FwdArgs.cseg, ApplyArgs.cseg)
  bool uc_list;     // the samples of every category are listed (k_uc_fill; FwdArgs.uc_by_sample, ApplyArgs.uc_list)
  bool usort;       // the user side from a sort of the batch's ids (UsortArgs)
  bool isort;       // the item side from a partitioned counting sort of the batch's ids (IsortArgs)
  bool rank;        // a ranking of the batch for the fused kernel's workgroups is written (BalArgs.perm)
  int by_window;    // ... in this form (BalArgs.by_window)
  int sparse;       // ScanArgs.sparse: the tables whose consumers reach the index through ids and records only
  int nthr;         // use slots of the batch: B (Ls + Sn + 1)
};
// The index plan plus what the step's launch adds (plan_front; the evaluation forward: plan_forward, no index).
struct FrontPlan {
  IndexPlan ix;
  int grp;          // samples per workgroup pass of the fused kernel (= per partial record)
  int ngroups;      // passes: ceil(B / grp)
  bool small;       // the pair's small-group kernel (Pair::fwd_bwd_small)
  bool lstream;     // the windows are streamed (longer than TLSAN_LS_MAX)
  bool fuse_dk;     // the dK product rides in the fused kernel (no k_dk_partial launch)
  int nsplit;       // dK partials the finalize sums
  int grid;         // workgroups of the fused kernel
  bool read_rank;   // the step deals the batch out by the index's ranking
};
// What the rules can ask of the buffers, at most, for a table shape and a largest batch (plan_capacity).
struct Capacity {
  bool lstream;     // workspace: the windows are streamed (gStat)
  bool cseg;        // workspace: Gc holds a row per item use as well (category segments)
  int kp_slots;     // workspace: dK partial matrices
  int max_records;  // workspace: partial records of a fused launch
  // the state's (they do not depend on the batch):
  bool isort;       // the item sort's buffers exist
  int rank_cap;     // samples of the largest batch that is ranked (St.perm)
  int uc_list_cap;  // samples of the largest batch whose categories are listed (St.uc_list)
};

// The training step's tail: the launches after the fused forward / backward kernel (run_backward), planned ONCE per step by
// plan_tail and issued by launch_tail.  The finalize launch and the second launch take the same ApplyArgs (TailPlan::fin.A):
// k_finalize_update writes per-workgroup S_delta records and hdr->spart_n laid out by nbH, nbC, nbI and nbU, and
// k_spec_commit walks its blocks by the same four counts.
enum TailForm {
  TAIL_APPLY,        // k_dense_finalize, then k_apply over every row (dense L2, tlsan_grads with full gradients)
  TAIL_SPLIT,        // row sums beside the finalize (k_finalize_presum), then k_update_lazy (sparse tlsan_grads: k_rc64_to_float)
  TAIL_SPEC,         // the speculative one pass: k_finalize_update, then k_spec_commit -- or nothing (TailPlan::two)
  TAIL_SPEC_SHARED,  // the same, the shared categories summed beside it and updated by the commit (k_*<.., CSPL>)
};
struct TailPlan {
  TailForm form;
  bool update;         // a train step (not tlsan_grads)
  FinLaunch fin;       // the finalize launch; run_backward fills the front half's fields of fin.f
  dim3 grid;           // the second launch's (TAIL_APPLY: launch_apply's own)
  bool wide;           // TAIL_SPLIT / TAIL_SPEC*: the second launch's wide row form
  int nbC16;           // TAIL_SPLIT update: k_update_lazy's blocks of 16 category rows
  // TAIL_SPEC, the two-launch form: no second launch.  The finalize's workgroups store the dense parameters and its summary
  // commits P and nstep; a clipped step's correction runs at the head of the next step's fused kernel, or in k_spec_flush
  // (tlsan_state_flush) when something else comes first.  run_backward hands the fused kernel the state's header for it.
  bool two;
};

#pragma GCC visibility push(hidden)
static inline bool apply_wide(int di, int dc, int WU) { return di > 64 || dc > 64 || WU > 128; }  // more float4 chunks per lane
static inline bool apply_wide(const ApplyArgs& A) { return apply_wide(A.di, A.dc, A.WU); }
// the tail walks the index's used-row records (a lazy-L2 step; tlsan_grads' per-row sums, out_sparse = tlsan_grads_out.sparse):
// the `sparse` of plan_index / plan_front
bool plan_sparse(const tlsan_hparams* hp, bool update, int out_sparse);
IndexPlan plan_index(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, bool sparse);
FrontPlan plan_front(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, const tlsan_hparams* hp, bool sparse);
FrontPlan plan_forward(const tlsan_dims* d, const Shape& s, const tlsan_batch* b);
Capacity plan_capacity(const tlsan_dims* d, const Shape& s, int B);
int plan_tail(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, const tlsan_hparams* hp, const Ws& w,
              const ApplyArgs& A0, bool update, TailPlan* P);
#pragma GCC visibility pop

// tlsan_tail.h -- the plan of a training step's tail, between the unit that makes it (tlsan_api_tail.hip) and the unit
// that issues it (tlsan_api.hip).
#pragma once
#include "tlsan_host.h"
#include "tlsan_update_inst.h"

// The training step's tail: the launches after the fused forward / backward kernel (run_backward), planned ONCE per step by
// plan_tail and issued by launch_tail.  The finalize launch and the second launch take the same ApplyArgs (TailPlan::fin.A):
// k_finalize_update writes per-workgroup S_delta records and hdr->spart_n laid out by nbH, nbC, nbI and nbU, and
// k_spec_commit walks its blocks by the same four counts.
enum TailForm {
  TAIL_APPLY,        // k_dense_finalize, then k_apply over every row (dense L2, tlsan_grads with full gradients)
  TAIL_SPLIT,        // row sums beside the finalize (k_finalize_presum), then k_update_lazy (sparse tlsan_grads: k_rc64_to_float)
  TAIL_SPEC,         // the speculative one pass: k_finalize_update, then k_spec_commit
  TAIL_SPEC_SHARED,  // the same, the shared categories summed beside it and updated by the commit (k_*<.., CSPL>)
};
struct TailPlan {
  TailForm form;
  bool update;         // a train step (not tlsan_grads)
  bool sparse_index;   // the tail walks the index's used-row records (build_index)
  FinLaunch fin;       // the finalize launch; run_backward fills the front half's fields of fin.f
  dim3 grid;           // the second launch's (TAIL_APPLY: launch_apply's own)
  bool wide;           // TAIL_SPLIT / TAIL_SPEC*: the second launch's wide row form
  int nbC16;           // TAIL_SPLIT update: k_update_lazy's blocks of 16 category rows
};

#pragma GCC visibility push(hidden)
static inline bool apply_wide(const ApplyArgs& A) { return A.di > 64 || A.dc > 64 || A.WU > 128; }  // more float4 chunks per lane
int plan_tail(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, const tlsan_hparams* hp, const Ws& w,
              const ApplyArgs& A0, bool update, TailPlan* P);
#pragma GCC visibility pop

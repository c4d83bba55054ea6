// tlsan_state.h -- the head of the persistent state buffer (StateHdr), which every stage of a training step reads or
// writes, and the per-workgroup records of the stored tables' sum of squares (DeltaRec).  Structures and constants only.
#pragma once
#include "tlsan_common.h"
#include <cstddef>

// index slots of the state: the batch being trained and up to two announced successors (tlsan_batch_index)
#define TLSAN_INDEX_SLOTS 3
// first bytes of the persistent state buffer
struct StateHdr {
  // ---- read-mostly line
  float P;                 // scale of the four regularised tables: W_true = P * W_stored (1 unless lazy L2)
  float P_prev;            // P before the current step's commit: what k_apply scales with
  int32_t n_uniq[TLSAN_INDEX_SLOTS][2];    // [index slot][item, user]: rows that received a gradient (k_index_scan)
  double St;               // sum of squares of the four STORED tables (true value: P^2 * St)
  float coef;              // global-norm clip coefficient of the current step (model.py:201)
  uint32_t nstep;          // update steps taken (salt of the stochastic rounding of bf16 tables)
  int32_t spart_n[2];      // [step & 1]: leading records of that step's S_delta array (DeltaRec) its update may have written
  int32_t n_hot[TLSAN_INDEX_SLOTS];        // [index slot] item rows with more than AP_HOT uses (k_index_scan; listed in the state)
  uint32_t folded;         // the step (nstep) whose S_delta records are already part of St (a step is folded once)
  // the speculative one-pass lazy update (k_finalize_update / k_spec_commit): the step summary leaves the table scale
  // AFTER the step and the step's salt here; P and nstep themselves are committed by the second launch, so that both
  // stay put while the first launch's row workgroups read them
  float P_next;
  uint32_t spec_salt;
  // the two-launch form of that update (FinArgs.spec == 2: no commit launch).  The step summary commits P and nstep itself,
  // so the row workgroups beside it read the SNAPSHOT of both that k_fwd_bwd of the same step left (workgroup 0, at its
  // start).  fix_pending != 0: the step was clipped (coefficient != 1, non-finite included) and its rows and dense
  // parameters still hold the speculative values -- corrected at the head of the next k_fwd_bwd (spec_fix_head,
  // tlsan_attn.h) or by k_spec_flush (tlsan_state_flush), from the step's ApplyArgs kept in the state (St::fix_args)
  float P_snap;
  uint32_t nstep_snap;
  uint32_t fix_pending;
  uint32_t fix_failed;     // != 0: a k_fwd_bwd gave up waiting for the correcting workgroups (it also left P = NaN: the step's loss and every later one are non-finite)
  float pad0[8];
  // ---- its own 128-B line: hammered by atomics, must not share a line with anything that is read
  int32_t ticket;          // arrival counter of k_dense_finalize: the last workgroup writes the step summary
  int32_t fix_arrive;      // correcting workgroups of k_fwd_bwd that are done (zeroed by the summary that sets fix_pending)
  int32_t fix_ticket;      // arrival counter of k_spec_flush: its last workgroup clears fix_pending
  int32_t pad1[29];
};
static_assert(sizeof(StateHdr) == 256, "StateHdr layout");
static_assert(offsetof(StateHdr, St) == 32, "StateHdr layout: St is read at byte 32 (tests/test_gpu_parity.py)");

// A workgroup's change of the stored tables' sum of squares, tagged with the step that made it (StateHdr::nstep after
// that step).  The next step's finalize adds up the records of the previous step, once (StateHdr::folded), and ignores
// older ones: nothing is ever cleared.  (Round 2 kept plain doubles that the finalize cleared as it consumed them;
// tlsan_state_renorm then rescaled a sum that lacked the last step's changes.)
// S_delta holds two arrays of nrec records (St::nrec), one per step parity: a record tagged t lives in array t & 1
// (delta_recs).  The fold of step t reads array t & 1 while the writers of step t + 1 -- in k_finalize_update, the same
// launch -- fill the other one, so no writer can overwrite a record before it is folded.
struct DeltaRec {
  double v;
  unsigned long long tag;
};
template <class R>
__device__ __forceinline__ R* delta_recs(R* base, int nrec, unsigned long long tag) { return base + (tag & 1) * (size_t)nrec; }

// (row-geometry limits, here because the index that ranks the hot rows and the apply stage that sums them both need them)
#define AP_HOT 48        // item rows with more uses than this are summed by a workgroup of their own ...
#define AP_HOT_CAP 64    // ... when there are at most this many (the head of a Zipf distribution: a handful)

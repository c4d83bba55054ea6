// tlsan_update_args.h -- the arguments and host-visible constants of everything after the fused forward / backward
// kernel: the dK product's split, the dense finalize (FinArgs), the row updates in all their forms (ApplyArgs) and one
// launch of the finalize (FinLaunch).  What the host units plan and fill in; no kernel.
#pragma once
#include "tlsan_state.h"

#define DK_WAVES 4   // wavefronts per workgroup: 4 -> 64 splits x (D/64)^2 quadrants = 256 workgroups at B = 4096, one
                                 // wavefront per SIMD on every CU (8 left half the chip idle with two wavefronts per SIMD)
#define DK_SPLITS_MAX (256 / DK_WAVES)
// (D = 256: sixteen quadrants per split and 64 KB of LDS per workgroup, two per CU -- at most 32 splits, so that the
//  launch's 512 workgroups are resident at once; with 64 it ran in two rounds: d = 256, Ls = 10 177 -> 175 us/step, bf16 139.6 -> 136.8)
static inline int dk_nsplit(int B, int D) {
  const int cap = D > 128 ? DK_SPLITS_MAX / 2 : DK_SPLITS_MAX;
  const int n = (B + DK_WAVES * 16 - 1) / (DK_WAVES * 16);
  return n < cap ? n : cap;
}
static inline int dk_spw(int B, int D) { const int per = (B + dk_nsplit(B, D) * DK_WAVES - 1) / (dk_nsplit(B, D) * DK_WAVES); return (per + 3) / 4 * 4; }
#define DK_SMEM_BYTES (DK_WAVES * 64 * 64 * 4)

#ifndef TLSAN_KCH
#define TLSAN_KCH 64     // dK partials a finalize thread has in flight (dense_finalize_block)
#endif
#define FIN_SMALL_PB 64  // small dense parameters per finalize workgroup (dense_finalize_block; the host's nbS)
#ifndef FIN_SMALL_KCH
#define FIN_SMALL_KCH 16 // records a lane has in flight there
#endif

// ------------------------------------------------------------------------------------------
struct FinArgs {
  tlsan_dense_layout lay;
  const float* partials;  // [nrec][NPB]
  int32_t nrec;
  const float* Kp;        // [nsplit][D*D]
  int32_t nsplit;
  float* gd;              // [n_dense] reduced dense gradients
  float* sqd;             // [nbK + nbS] per-block sum of gd^2
  float* scal;            // [0] = sum of per-sample BCE, [1] = sum of squares of per-use rows
  const DeltaRec* S_delta; // per-workgroup changes of the regularised tables' sum of squares, tagged by step
  int32_t delta_nrec;      // records per step-parity array of S_delta (DeltaRec)
  double* S_total;
  // step summary (written by the last workgroup to arrive)
  StateHdr* hdr;
  float lr, reg, clip, inv_B;
  int32_t norm_mode;
  int32_t commit;          // lazy L2 update: advance the table scale P (P_prev keeps the old value)
  int32_t count_step;      // an update follows (train step, not tlsan_grads): advance hdr->nstep
  int32_t spec;            // speculative one-pass lazy update: neither P nor nstep are touched here (commit = count_step = 0);
                           // the scale after the step and the step's salt go to hdr->P_next / hdr->spec_salt (k_spec_commit)
                           // 2: the two-launch form -- no commit launch follows.  The finalize workgroups store the dense
                           // parameters with coefficient 1 as they reduce their gradients (spec_w / spec_wKT), and the
                           // summary commits P and nstep and says whether a correction is due (hdr->fix_pending)
  float* spec_w; float* spec_wKT;   // spec == 2: tlsan_params.dense / dense_KT
  float* out_loss; float* out_gnorm; float* out_sq;
};

// ------------------------------------------------------------------------------------------
enum { AP_UPDATE = 0, AP_GRADS = 1, AP_SUMSQ = 2, AP_ROWNORM = 3,
       AP_PRESUM = 4 };  // PRESUM: only the exact per-row sums, left in Rc / Ri / Rb / Ru for k_update_lazy

struct ApplyArgs {
  tlsan_params p;
  tlsan_grads_out go;
  tlsan_dense_layout lay;
  int32_t I, U, C, Ls, D, di, dc, WU;
  const float* Gi; const float* Gb; const float* Gu; const float* Gc;
  int32_t* cnt_item; int32_t* cnt_user; int32_t* cnt_uc;
  const int32_t* off_item; const int32_t* off_user; const int32_t* off_uc;   // n+1 entries each
  const int4* urec_item; const int4* urec_user;   // lazy L2: (row, first position, uses) of the rows used this step
  const int32_t* cate_off; const int32_t* cate_cnt; const int32_t* cate_items;  // static CSR
  const int32_t* uc_list;  // optional: samples of every category (segments off_uc); then Gc is in sample order
  int32_t cseg;            // != 0 (many categories): a category's segment of Gc holds its u_cate uses AND the category halves
                           // of its items' uses (k_fwd_bwd, FwdArgs.cseg): the category blocks sum that one segment and
                           // do not walk the category's items
  const float* gd;
  float* Rc; float* Ri; float* Rb; float* Ru;   // PRESUM -> k_update_lazy: summed rows [C][dc], [slot][di], [slot], [slot][WU]
  int32_t presum_rows;     // PRESUM: write the item / user sums to the rows of `go` instead (tlsan_grads with reg = 0)
  // PRESUM with few, large categories (Movies-TV: 15): csplit > 1 workgroups share a category (each takes
  // every csplit-th pass of cpass items and its share of the u_cate uses) and add their exact partial
  // sums into Rc64 with double atomics --
  // sums of 2^-40-grid values are exact in any order, so the result stays bitwise reproducible;
  // k_update_lazy rounds them to float (as a single workgroup would have) and clears them
  int32_t csplit, cpass;
  // cpos != 0 (categories of at most 256 items -- one pass): the sharing workgroups all scan the category's items and
  // each takes an equal slice of the concatenated USE POSITIONS instead of every csplit-th group of items: a hot item no
  // longer makes its share the launch's longest chain (Digital-Music, batch 2048: one share 14 us, the rest 7)
  int32_t cpos;
  // hot item rows (more than AP_HOT uses) get a workgroup each in the row-sum pass: nbH = AP_HOT_CAP such
  // workgroups lead the grid, the item-row workgroups leave those rows to them (when the list did not overflow)
  const int32_t* hot_n; const int32_t* hot_list; int32_t nbH;
  int32_t delta_nrec;      // UPDATE: records per step-parity array of delta_out (DeltaRec)
  double* Rc64;            // [C][dc], zero at rest (state)
  double* part_out;        // SUMSQ: sum of squares per workgroup; ROWNORM: sum g^2
  DeltaRec* delta_out;     // UPDATE: change of the stored tables' sum of squares per workgroup, tagged with the step (S_delta)
  StateHdr* hdr;           // P, P_prev, coef (read); spart_n (written by an update)
  const int32_t* n_uniq_item; const int32_t* n_uniq_user;   // used-row counts of this step's index slot
  float lr, reg;
  int32_t nbI, nbU, nbC, nbD;
  // k_finalize_update: item-row workgroups LAUNCHED (0: nbI).  The host sizes nbI for the most rows the batch can touch
  // (C5: 25.8 k blocks of 16 rows; 4.4 k are real, the rest start, find nothing and leave -- 5 us of the launch's slots);
  // with nbI_l < nbI a workgroup takes the blocks nbI_l apart until the used rows end
  int32_t nbI_l;
  int32_t ufirst;          // k_finalize_update: the user-row workgroups lead the item-row workgroups
  // k_finalize_update, two-launch form (FinArgs.spec == 2): where the launch leaves a copy of these arguments for the
  // correcting pass of a clipped step (spec_fix_blocks), which runs in a later launch; NULL: the three-launch form
  void* fix_args;
  // optimizers other than SGD (dense UPDATE only): accumulator tables shaped like p, see tlsan_optimizer
  tlsan_params s1, s2;
  int32_t opt;
  float ob1, ob2, oeps, oalpha;   // oalpha: Adam's lr * sqrt(1 - beta2^t) / (1 - beta1^t)
  unsigned long long* stamps;  // debug: 8 s_memtime stamps per workgroup (tlsan_debug_stamps)
};

#define AP_OWN 8        // uses a 16-lane group sums alone before the wavefront helps
#define AP_ROWS_PB 16   // item / user rows per workgroup (4 wavefronts x 4 groups)

// the speculative one-pass update (tlsan_finalize_rows.h): rows in flight per 16-lane group (wide form); correcting workgroups
#ifndef SPEC_OWN
#define SPEC_OWN 2
#endif
#define SPEC_FIX_BLOCKS 512
#define SPEC_ITEM_BLOCKS 2048   // item-row workgroups k_finalize_update launches at most (ApplyArgs.nbI_l)

struct FinLaunch {   // one launch of the dense finalize, in any of its three forms (tlsan_update_inst.h: launch_finalize)
  enum Kind { DENSE = 0, PRESUM = 1, UPDATE = 2 };
  FinArgs f;
  ApplyArgs A;       // PRESUM, UPDATE: the row workgroups of the launch
  dim3 grid;
  int nbK, nbS;
  int kind;
  bool shared;       // UPDATE: shared categories (plan_tail: TAIL_SPEC_SHARED)
  bool bf16;         // UPDATE: bf16 tables
  bool wide;         // PRESUM, UPDATE: the wide row form
  bool low;          // UPDATE: the low-occupancy form (tables in HBM)
  bool csplit;       // PRESUM: categories split over several workgroups
};

// tlsan_api_tail.hip -- which form the tail of a training step takes (plan_tail): the launches after the fused forward /
// backward kernel, their grids and the split of the categories, decided once per step from the shapes and the measured
// rules below.  Host code only; tlsan_api.hip issues the plan (launch_tail).
#define TLSAN_ONCE static   // (the kernels of tlsan_update.h that are not templates: tlsan_api.hip's)
#include "tlsan_tail.h"

// lazy (UPDATE only): the row blocks walk the compacted records of used rows.
static void lazy_blocks(ApplyArgs& A, int B, int Sn) {  // at most min(rows, uses) rows were used
  const long ni = (long)B * (A.Ls + Sn + 1);
  A.nbI = (int)(((ni < A.I ? ni : A.I) + AP_ROWS_PB - 1) / AP_ROWS_PB);
  A.nbU = ((B < A.U ? B : A.U) + AP_ROWS_PB - 1) / AP_ROWS_PB;
}

// few, large categories: several workgroups per category in the row-sum pass, every one with its share of the items and of the
// u_cate uses (estimated from the batch shape; up to 64 per category).
//  * from 512 uses per category on: about 128 uses per workgroup (round 3; Movies-TV's 15 categories at batch 4096), within
//    a budget of ~700 category workgroups (round 6, below);
//  * round 6 -- where the launch has SLOTS TO SPARE (its other workgroups and the category workgroups all resident at once:
//    small batches), from ~100 uses on and ~48 per workgroup: a category workgroup is a chain of dependent trips (3 us
//    before its first gradient row arrives) plus ~0.03 us per use, and such a launch ends with its longest chain --
//    Digital-Music's 53 categories at batch 1024 (300 uses each) took 9-13 us where everything else had finished after 7:
//    51.4 -> 48.2 us/step.  Where the launch is bound by slots (batch 4096: the bench's 673 categories of ~100 uses,
//    Movies-TV) every workgroup more costs its lead-in again: 64 instead of 46 per category at Movies-TV, Ls = 10:
//    59.1 -> 61.5 (profiles/r06_ab_csplit.txt).
// TLSAN_CSPLIT_FINE=0 (read once): the first rule only (A/B).
static void category_split(ApplyArgs& A, const tlsan_dims* d, const tlsan_batch* b) {
  // category segments (A.cseg) sum a category as ONE contiguous segment, 16 categories per workgroup
  // (apply_cseg_block): there is nothing to split, and the split kernels decode blocks as (category, share)
  if (A.cseg) return;
  const long uses = ((long)b->B * (d->Ls + b->Sn + 2) + d->cate_count - 1) / d->cate_count;
  const int per = (d->item_count + d->cate_count - 1) / d->cate_count;
  static const int fine = [] { const char* e = getenv("TLSAN_CSPLIT_FINE"); return e ? atoi(e) : 1; }();
  // (the first rule's budget of category workgroups, round 6: every share repeats the category's lead-in, and a launch
  //  bound by slots pays for it 1:1 -- 673 categories of 620 uses (Ls = 90) as four shares each: 2 692 workgroups of 8.8 us,
  //  24 of the launch's 32 k slot-us; unshared: d = 256 239 -> 224 us/step, d = 128 103.5 -> 97.4.  Movies-TV's 15
  //  categories run best as ~46 shares each at Ls = 10 AND at Ls = 90 (64: 97.7, 46: 94.4, 30: 94.9, 11: 104), i.e. ~700
  //  category workgroups beside the rows' on 1 280 slots.)
  long n = uses > 512 ? (uses / 128 < 64 ? uses / 128 : 64) : 1;
  if (n > 700 / d->cate_count) n = 700 / d->cate_count;
  if (n < 1) n = 1;
  if (fine && uses > 96) {
    // the launch's other workgroups: the finalize's and the hot rows' (~206), 16 used item / user rows each (lazy_blocks)
    const long ni = (long)b->B * (d->Ls + b->Sn + 1);
    const long others = 206 + ((ni < d->item_count ? ni : d->item_count) + 15) / 16 + ((b->B < d->user_count ? b->B : d->user_count) + 15) / 16;
    long nf = uses / 48 < 64 ? uses / 48 : 64;
    const long spare = (1280 - others) / d->cate_count;     // (256 CUs x five 256-thread workgroups)
    if (nf > spare) nf = spare;
    if (nf > n) n = nf;
  }
  if (n > 1) {
    A.csplit = (int)n;
    const int ps = (per + A.csplit - 1) / A.csplit;
    A.cpass = ps < 1 ? 1 : (ps > 256 ? 256 : ps);
    // categories of at most 256 items (one pass of the walk: the static CSR's counts, not the average, would say; the
    // kernel takes further passes the same way if one is larger): shares by use position instead of by item, so that a
    // hot item does not make its share the launch's longest chain.  TLSAN_CSPLIT_POS=0: by item (A/B)
    static const int by_pos = [] { const char* e = getenv("TLSAN_CSPLIT_POS"); return e ? atoi(e) : 1; }();
    A.cpos = (by_pos && per <= 128) ? 1 : 0;
  }
}

// The lazy update as ONE pass over the used rows (round 6; k_finalize_update / k_spec_commit, tlsan_update.h).  The split
// form (row sums in the finalize's launch, then k_update_lazy) sends every summed row through memory -- written by one
// launch, read by the next beside the parameter row's read-modify-write -- and ends in a launch of its own; in the one-pass
// form a 16-lane group sums its row's segment and updates the row, speculating on clip coefficient 1, beside the finalize.
static bool tables_in_hbm(const tlsan_dims* d) {      // (well beyond the 256 MiB Infinity Cache)
  return 4.0 * ((double)d->item_count * d->d_item + (double)d->user_count * (d->d_item + d->Ls)) > 512e6;
}

// A: fill_apply's (+ tlsan_grads' outputs, the optimizer's slots).  update: a train step; otherwise tlsan_grads.
int plan_tail(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, const tlsan_hparams* hp, const Ws& w,
                     const ApplyArgs& A0, bool update, TailPlan* P) {
  ApplyArgs A = A0;
  *P = TailPlan{};
  FinLaunch& fl = P->fin;
  FinArgs& f = fl.f;
  f.gd = w.gd; f.count_step = update ? 1 : 0;
  fl.nbK = w.nbK; fl.nbS = w.nbS;
  P->update = update;
  const bool lazy = update && hp->l2_mode == TLSAN_L2_LAZY;
  // lazy Adam / RMSProp / Adadelta (TLSAN_OPT_LAZY): always the split form -- the one-pass forms speculate on the clip
  // coefficient and correct linearly, which a non-linear update cannot -- and the table scale stays 1 (no commit)
  const bool lazy_opt = lazy && A.opt != TLSAN_OPT_SGD;
  // tlsan_grads' pure per-row sums of the used rows (what the sharded step asks for): they ride with the dense finalize as in
  // the lazy train step, written straight to the output rows -- no apply launch (sparse == 2: the four outputs are views of
  // ONE fused row table, see tlsan_grads_out)
  const bool sparse_grads = !update && A.go.sparse && hp->reg == 0.0f && hp->norm_mode == TLSAN_NORM_TF18;
  P->sparse_index = lazy || sparse_grads;
  if (!P->sparse_index) {
    P->form = TAIL_APPLY;
    fl.kind = FinLaunch::DENSE; fl.grid = dim3(w.nfin + 1); fl.A = A;
    return TLSAN_OK;
  }
  if (sparse_grads) { A.presum_rows = A.go.sparse == 2 ? 2 : 1; A.Rc = A.go.cate_emb; f.gd = A.go.dense; }
  category_split(A, d, b);
  lazy_blocks(A, b->B, b->Sn);
  A.nbH = AP_HOT_CAP;   // hot item rows: a workgroup each, leading the row workgroups (they return at once where there are none)
  const bool bf16 = A.p.table_dtype == TLSAN_TABLE_BF16;
  // Where the one-pass form was measured to win (profiles/r06_lazy_one_pass.md): rows of up to 64 floats per table half
  // (d <= 128) at any table size -- bench shape 56.9 -> 55.4 us/step, 8192 sequences 106.5 -> 103.6, Amazon session lengths
  // 59.9 -> 57.8, 10 M / 5 M tables 97 -> 80 --; wider rows (d = 256) only where the tables live in HBM (C5 300 -> 267; with
  // cache-resident tables it loses 2.5 us to the split form).  TLSAN_LAZY_ONE_PASS: 0 never, 1 (default) as described,
  // 2 whenever the tables take category segments, 3 wherever the form is built.
  // TAIL_SPEC_SHARED: one pass over the item and user rows while the category rows -- few, large categories (Movies-TV: 15)
  // that several row-sum workgroups share, adding exact doubles with atomics (category_split) -- are summed beside them and
  // updated by the commit launch (k_finalize_update / k_spec_commit<.., CSPL>).
  static const int mode = [] { const char* e = getenv("TLSAN_LAZY_ONE_PASS"); return e ? atoi(e) : 1; }();
  // bf16 tables: a clipped step rounds twice in the one-pass form -- the speculative write at the magnitude of w - lr g, the
  // correction at that of the result -- so its stored elements can be off by one ulp of the SPECULATIVE value (unbiased,
  // and only in clipped steps; fp32 tables: 2^-24 of it, far inside every bound).  Taken where it pays for that (tables in
  // HBM: C5 in bf16 227 -> 202 us/step); with cache-resident bf16 tables (0.4-1.0 us) the split form and its
  // one-rounding guarantee stay.
  const bool cache_bf16 = bf16 && !tables_in_hbm(d);
  TailForm form = TAIL_SPLIT;
  if (lazy && !lazy_opt && mode != 0) {
    if (A.csplit > 1) {   // (built in the narrow form: d <= 128)
      if (mode != 2 && A.di <= 64 && A.dc <= 64 && A.WU <= 256 && !(mode == 1 && cache_bf16)) form = TAIL_SPEC_SHARED;
    } else if (A.cseg || !apply_wide(A)) {   // (the wide form is built for category segments only)
      if (mode >= 2) form = (mode != 2 || A.cseg) ? TAIL_SPEC : TAIL_SPLIT;
      else if (!cache_bf16 && (!apply_wide(A) || tables_in_hbm(d))) form = TAIL_SPEC;
    }
  }
  P->form = form;

  if (form == TAIL_SPLIT) {
    // the exact row sums of the apply pass share the finalize's launch (they wait for nothing it produces)
    A.nbC = A.cseg ? (A.C + AP_ROWS_PB - 1) / AP_ROWS_PB : A.C * A.csplit;
    fl.kind = FinLaunch::PRESUM;
    fl.grid = dim3(w.nfin + 1 + A.nbH + A.nbC + A.nbI + A.nbU);
    // (the row-sum launch covers user rows of up to 256 floats in two passes of its narrow form -- 92 registers, five
    //  workgroups per CU, instead of 135 and three; the sharded step's fused rows keep the wide form.  d = 128 with 90-entry
    //  windows: Movies-TV shape 106.6 -> 104.3 us/step, with 673 categories 116.2 -> 106.2: profiles/r04_presum_narrow_ab.md)
    fl.wide = A.di > 64 || A.dc > 64 || (A.WU > 128 && A.presum_rows != 0);
    fl.csplit = A.csplit > 1;
    f.commit = lazy && !lazy_opt ? 1 : 0;
    if (lazy) {   // k_update_lazy (_opt): ceil(C / 16) blocks of category rows, the used item / user rows, the dense parameters
      P->nbC16 = (A.C + 15) / 16;
      P->grid = dim3(P->nbC16 + A.nbI + A.nbU + A.nbD);
      P->wide = apply_wide(A);
    } else {      // k_rc64_to_float (split categories only)
      P->grid = dim3((A.C * A.dc + 255) / 256);
    }
  } else {
    // the row workgroups UPDATE beside the finalize, with clip coefficient 1 (k_finalize_update); the commit and -- after a
    // clipped step -- the correction follow in k_spec_commit
    const bool shared = form == TAIL_SPEC_SHARED;
    if (shared && s.D > 128) return fail(TLSAN_E_UNSUPPORTED, "shared categories in the one-pass update: d <= 128");
    // (shared: A.nbC = the commit launch's blocks of 16 category rows; the finalize's launch carries C * csplit)
    if (shared) A.nbC = (A.C + 15) / 16;
    // (item-row workgroups launched: at most SPEC_ITEM_BLOCKS -- ApplyArgs.nbI_l; TLSAN_SPEC_ITEM_BLOCKS=<n>, 0: all.  The
    //  shared-category form keeps SPEC_ITEM_BLOCKS -- Movies-TV's 1787 blocks stay below it; fewer, 1024 / 640 / 384,
    //  measured a loss there: profiles/r06_ab_hot_cate.txt)
    static const int item_cap = [] { const char* e = getenv("TLSAN_SPEC_ITEM_BLOCKS"); return e ? atoi(e) : SPEC_ITEM_BLOCKS; }();
    const int cap = shared ? SPEC_ITEM_BLOCKS : item_cap;
    A.nbI_l = (cap > 0 && A.nbI > cap) ? cap : 0;
    // user-row workgroups ahead of the item rows in the wide form (profiles/r06_ab_c5_tail.txt); shared categories: where the
    // user rows take two passes of the narrow form (k_finalize_update<.., CSPL>)
    A.ufirst = (shared ? A.WU > 128 : apply_wide(A)) ? 1 : 0;
    fl.kind = FinLaunch::UPDATE;
    fl.grid = dim3(w.nfin + 1 + A.nbH + (shared ? A.C * A.csplit : A.nbC) + (A.nbI_l > 0 ? A.nbI_l : A.nbI) + A.nbU);
    fl.shared = shared; fl.bf16 = bf16; fl.wide = apply_wide(A) && !shared;
    fl.low = tables_in_hbm(d);   // (the low-occupancy form: see SPEC_WPE, tlsan_update.h)
    f.count_step = 0; f.spec = 1;
    // k_spec_commit: the dense parameters, (shared: the category-row blocks,) then at most SPEC_FIX_BLOCKS correcting workgroups
    const int nrow = A.nbH + (shared ? 0 : A.nbC) + A.nbI + A.nbU;
    P->grid = dim3(A.nbD + (shared ? A.nbC : 0) + (nrow < SPEC_FIX_BLOCKS ? nrow : SPEC_FIX_BLOCKS));
    P->wide = fl.wide;
  }
  fl.A = A;
  return TLSAN_OK;
}

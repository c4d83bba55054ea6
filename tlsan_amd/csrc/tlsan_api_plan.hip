// tlsan_api_plan.hip -- the plans of a training step, each decided once per step from the shapes and the measured rules
// below.  The front (plan_index, plan_front): what the destination index holds, the fused forward / backward kernel's
// geometry and where the dK product runs.  The tail (plan_tail): the launches after the fused kernel, their grids and the
// split of the categories.  The buffers those rules can ask for (plan_capacity).  Host code only, and every environment
// switch of the library is read here; tlsan_api.hip issues the plans (build_index, run_backward, launch_tail).
#include "tlsan_plan.h"
#include "tlsan_index_args.h"

// ================================================================ the front ================================================
// windows longer than TLSAN_LS_MAX are streamed (the list form of the long block); shorter ones stay in registers
static bool streamed(int Ls) { return Ls > TLSAN_LS_MAX; }

// the dK product rides in k_fwd_bwd for D <= 128 (Geo::FUSE_DK); its launch then has at most this many workgroups
// (each loops over its passes), so that the per-workgroup partials stay a few tens of MB at any batch size
// ... when there is at most one partial per CU: more of them (d = 64 at 8192 sequences: 512) make the reduction in
// k_dense_finalize the long pole of its launch (77 -> 91 us/step), and the separate k_dk_partial launch (<= 64 partials)
// is the better deal again
#define FUSED_DK_MAX_GROUPS 256
static bool fused_dk(int D, int ngroups) { return D <= 128 && ngroups <= FUSED_DK_MAX_GROUPS; }

// Samples per workgroup pass of a TRAINING launch of the fused kernel (= per partial record): the width's NSB, or the
// pair's small pass (Shape::SG: 8 at d = 128 with 8 heads, 4-wavefront workgroups: Geo<128, 16, 4>) with the window in
// registers and no dropout, when the batch is so small that 16-sample workgroups would leave three quarters of the CUs
// idle -- a wavefront then runs alone on its SIMD (profiles/r04_nw4_ab.md; at larger batches the 16-sample workgroups are
// faster).  hp NULL: a launch without dropout (what the index is planned for, see plan_front).
// TLSAN_NW4 (A/B measurements; read once): 0 never, 1 as described, 2 always.
static int train_group(const Shape& s, const tlsan_dims* d, const tlsan_batch* b, const tlsan_hparams* hp) {
  static const int mode = [] { const char* e = getenv("TLSAN_NW4"); return e ? atoi(e) : 1; }();
  if (!s.SG || streamed(d->Ls) || (hp && hp->dropout != 0.0f) || mode == 0) return s.NSB;
  if (mode == 1 && (b->B + s.NSB - 1) / s.NSB > 64) return s.NSB;
  return s.SG;
}

#define BAL_CAP (1 << 14)      // batches up to this many samples are ranked for the fused kernel's workgroups (BalArgs, tlsan_index_args.h)
// Streamed windows: a workgroup's time is proportional to its windows' total length (d = 64, Ls = 90: 98 -> 87 us/step;
// d = 256 at the C5 shape 496 -> 471; d = 128: the kernel alone 94 -> 72 us, 104 -> 93 beside the index build of the batch
// after next).  Windows in registers: evenly loaded workgroups (ranked by session length alone) ran no faster in round 4
// (bench 61.0 vs 61.1 us/step; Amazon session lengths 65.6 vs 66.2) -- the launch ends with the workgroups that hold one
// of the few long sessions, however they are dealt; what does help is giving THOSE workgroups the batch's shortest
// windows (round 5, BalArgs: bench 58.2 -> 57.15, Amazon session lengths 61.85 -> 59.05, d = 256 169.4 -> 162.0:
// profiles/r05_ab_bal_reg.txt).
// (round 5: windows in registers as well, with a ranking that gives the workgroups of the batch's longest sessions its
//  shortest windows -- BalArgs; TLSAN_BAL_REG=0: streamed windows only, as before)
static int bal_reg_mode() {   // 0 off, 1 on, 2 on without the reversed group numbering (A/B)
  static const int reg = [] { const char* e = getenv("TLSAN_BAL_REG"); return e ? atoi(e) : 1; }();
  return reg;
}
static bool balanced(const tlsan_dims* d, const tlsan_batch* b) {
  if (b->B <= 16 || b->B > BAL_CAP) return false;
  if (streamed(d->Ls)) return true;
  // windows in registers: where it was measured to win -- one round of workgroups (<= 256 groups of 16: a second round
  // evens the workgroups out by itself, and 16384 sequences ran 5 % SLOWER ranked: 207 vs 196 us/step) and tables that the
  // caches hold (10 M users / 5 M items: 101.7 vs 97.4 -- full windows side by side mean more HBM rows in flight at once);
  // profiles/r05_ab_bal_reg_shapes2.txt
  return bal_reg_mode() != 0 && b->Sn > 0 && (b->B + 15) / 16 <= FUSED_DK_MAX_GROUPS && d->item_count <= (1 << 18);
}

#define UC_LIST_CAP (1 << 18)  // batches up to this many samples may keep a per-category sample list in the state
// ... and do when a category sees many of the batch's samples (cursor atomics on few addresses inside the
// fused kernel cost more than the extra launch on the index stream): more than 32 samples per category
static bool uc_by_list(const tlsan_dims* d, const tlsan_batch* b) {
  return b->B <= UC_LIST_CAP && (long)b->B > 32L * d->cate_count;
}
// tables with at least this many categories take the category-segment path (cate_seg below; TLSAN_CSEG_MIN=<n> for tests
// and experiments, read once per process)
#define TLSAN_CSEG_MIN_CATES 2048
static int cseg_min_cates() {
  static const int v = [] { const char* e = getenv("TLSAN_CSEG_MIN"); return e ? atoi(e) : TLSAN_CSEG_MIN_CATES; }();
  return v;
}
// many categories (the 10 k of BASELINE.json configs[4]): the category half of every item use's gradient row is written
// into the category's own segment of Gc (FwdArgs.cseg) -- a category block of the apply pass then sums one contiguous
// segment instead of walking the category's items for their segments (500 items per category at 5 M items, of which a
// batch uses five: k_finalize_presum 196 us at that shape).  With few categories the cursor draws would pile up on few
// addresses (as the u_cate uses did, uc_by_list): the item walk stays.
// (the category counts of CSEG need the item -> category map: tlsan_batch_index takes it as an argument -- round 3 kept
//  a process-global registry state -> map filled by tlsan_state_init, which a re-allocated map or a recycled state
//  address left stale)
static bool cate_seg(const tlsan_dims* d, const tlsan_batch* b) {
  return d->cate_count >= cseg_min_cates() && !uc_by_list(d, b);
}
// Tables of at least this many rows take their side of a lazy-SGD step's index from a sort of the batch's ids instead of
// a counter per row -- when its consumers reach it through ids and records only: the user table (UsortArgs: a bucket
// sort inside one block), the item table with category segments (IsortArgs: a partitioned counting sort, tlsan_index.h).
// TLSAN_ISORT_MIN=<rows> for tests (read once per process; it also sizes the state).
static int isort_min_rows() {
  static const int v = [] { const char* e = getenv("TLSAN_ISORT_MIN"); return e ? atoi(e) : (1 << 16); }();
  return v;
}
static bool isort_rows_ok(int rows) { return rows >= isort_min_rows() && (long)rows <= (long)IS_MAXB * IS_BSZ; }

bool plan_sparse(const tlsan_hparams* hp, bool update, int out_sparse) {
  // tlsan_grads' pure per-row sums of the used rows (what the sharded step asks for): they ride with the dense finalize as in
  // the lazy train step, written straight to the output rows -- no apply launch (sparse == 2: the four outputs are views of
  // ONE fused row table, see tlsan_grads_out)
  return update ? hp->l2_mode == TLSAN_L2_LAZY : out_sparse && hp->reg == 0.0f && hp->norm_mode == TLSAN_NORM_TF18;
}

IndexPlan plan_index(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, bool sparse) {
  IndexPlan ix = {};
  ix.cseg = cate_seg(d, b);
  ix.uc_list = uc_by_list(d, b);
  ix.nthr = b->B * (d->Ls + b->Sn + 1);
  // a table's side from a sort of the batch's ids when only the used rows are wanted and the table is large: the user
  // table (UsortArgs); the item table (IsortArgs) when a lazy-SGD step with category segments consumes the index (it
  // reaches item offsets / cursors through ids and records only)
  ix.usort = sparse && b->B <= USORT_MAX && d->user_count >= isort_min_rows();
  ix.isort = sparse && ix.cseg && ix.nthr <= ISORT_MAX_SLOTS && isort_rows_ok(d->item_count);
  // the user table of a lazy-L2 SGD step: its consumers reach off / cur through the batch's ids or the used-row records
  // only (the dense sweeps and tlsan_grads read the offsets of every row)
  // (category segments: nothing walks the item offsets per category either -- 5 M items: 40 MB of writes per step less)
  ix.sparse = sparse ? ((1 << 2) | (ix.cseg ? 1 : 0)) : 0;
  // (no ranking block for a launch that will not read it -- the small-group workgroups of small d = 128 batches
  //  take the batch's own order: the ranking deals the batch out in groups of NSB)
  ix.rank = balanced(d, b) && train_group(s, d, b, nullptr) == s.NSB;
  if (ix.rank) ix.by_window = streamed(d->Ls) ? 1 : (bal_reg_mode() == 2 ? -1 : 0);
  return ix;
}

// The index may have been built one or two steps before the step, by tlsan_batch_index on another stream and without the
// step's hyper-parameters: it is planned for a launch without dropout (train_group(.., NULL)).  A step with dropout takes
// full-size groups where the index expected small ones -- and then finds no ranking; the reverse does not happen (dropout
// only ever turns small groups into full-size ones).  So the step reads the ranking if and only if the index wrote one and
// the launch takes full-size groups: both from the same IndexPlan, here.
FrontPlan plan_front(const tlsan_dims* d, const Shape& s, const tlsan_batch* b, const tlsan_hparams* hp, bool sparse) {
  FrontPlan f = {};
  f.ix = plan_index(d, s, b, sparse);
  f.grp = train_group(s, d, b, hp);
  f.ngroups = (b->B + f.grp - 1) / f.grp;
  f.small = f.grp != s.NSB;
  f.lstream = streamed(d->Ls);
  f.fuse_dk = fused_dk(s.D, f.ngroups);
  // dK partials: one per batch split of k_dk_partial, or (fused) one per workgroup of the fused launch, a pass each
  f.nsplit = f.fuse_dk ? f.ngroups : dk_nsplit(b->B, s.D);
  f.grid = f.ngroups < 4096 ? f.ngroups : 4096;
  f.read_rank = f.ix.rank && !f.small;
  return f;
}

// the evaluation forward: full-size groups in the batch's order, no index, no dK product
FrontPlan plan_forward(const tlsan_dims* d, const Shape& s, const tlsan_batch* b) {
  FrontPlan f = {};
  f.grp = s.NSB;
  f.ngroups = (b->B + s.NSB - 1) / s.NSB;
  f.lstream = streamed(d->Ls);
  f.grid = f.ngroups < 4096 ? f.ngroups : 4096;
  return f;
}

Capacity plan_capacity(const tlsan_dims* d, const Shape& s, int B) {
  Capacity c = {};
  c.lstream = streamed(d->Ls);
  // (CSEG: one row of Gc per u_cate use AND per item use -- sized for it whenever the table shape can take that path)
  c.cseg = d->cate_count >= cseg_min_cates();
  c.isort = isort_rows_ok(d->item_count);
  c.rank_cap = BAL_CAP;
  c.uc_list_cap = UC_LIST_CAP;
  // partial records: one per workgroup pass, of the smallest pass a launch may take (8 samples, Pair::small_grp -- kept
  // for every pair: the workspace's size is part of what a caller sees)
  c.max_records = (B + 7) / 8;
  // dK partials: one per batch split of k_dk_partial, or (fused into the forward/backward kernel, D <= 128) one per
  // workgroup of that launch -- which of the two, and how many, is the launch's choice (plan_front)
  // (sized so that the workspace of a batch also holds every smaller batch: the fused form of a smaller batch can
  //  need more partials than the split form of a larger one)
  c.kp_slots = dk_nsplit(B, s.D);
  if (s.D <= 128) {
    const int g = s.SG ? s.SG : s.NSB;     // (small groups: twice the groups)
    const int ng = (B + g - 1) / g;
    const int fmax = ng < FUSED_DK_MAX_GROUPS ? ng : FUSED_DK_MAX_GROUPS;
    if (fmax > c.kp_slots) c.kp_slots = fmax;
  }
  return c;
}

// ================================================================ the tail =================================================
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

// The lazy update as ONE pass over the used rows (round 6; k_finalize_update, tlsan_finalize_rows.h / k_spec_commit, tlsan_spec_commit.h).  The split
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
  const bool sparse = plan_sparse(hp, update, A.go.sparse);
  const bool lazy = update && sparse, sparse_grads = !update && sparse;
  // lazy Adam / RMSProp / Adadelta (TLSAN_OPT_LAZY): always the split form -- the one-pass forms speculate on the clip
  // coefficient and correct linearly, which a non-linear update cannot -- and the table scale stays 1 (no commit)
  const bool lazy_opt = lazy && A.opt != TLSAN_OPT_SGD;
  if (!sparse) {
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

  if (form != TAIL_SPEC) A.fix_args = nullptr;   // (fill_apply's: the two-launch form's alone)
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
    fl.low = tables_in_hbm(d);   // (the low-occupancy form: see SPEC_WPE, tlsan_finalize_rows.h)
    f.count_step = 0; f.spec = 1;
    // The two-launch form: everything k_spec_commit does has a place where its inputs are final at a launch boundary (the
    // finalize's workgroups, its summary, the head of the next fused kernel), so the launch -- 4.4 us of a 56 us step for
    // 17.6 k dense stores and two words -- goes.  Not with shared categories, whose rows the commit launch updates.
    // Not where the tables live in HBM either: there the step is bound by the index stream beside it, and at 10 M / 5 M rows,
    // d = 128 two launches LOSE 3 us of 78 in every one of five interleaved rounds (profiles/two_launch.md).
    // TLSAN_TWO_LAUNCH=0: the three-launch form everywhere (A/B, and the reference of the bit-equality test); 2: the
    // two-launch form for tables in HBM as well (the A/B of that loss).
    static const int two_launch = [] { const char* e = getenv("TLSAN_TWO_LAUNCH"); return e ? atoi(e) : 1; }();
    P->two = !shared && two_launch != 0 && (!fl.low || two_launch == 2);
    if (P->two) { f.spec = 2; f.spec_w = A.p.dense; f.spec_wKT = A.p.dense_KT; }
    else A.fix_args = nullptr;
    // k_spec_commit: the dense parameters, (shared: the category-row blocks,) then at most SPEC_FIX_BLOCKS correcting workgroups
    const int nrow = A.nbH + (shared ? 0 : A.nbC) + A.nbI + A.nbU;
    P->grid = dim3(A.nbD + (shared ? A.nbC : 0) + (nrow < SPEC_FIX_BLOCKS ? nrow : SPEC_FIX_BLOCKS));
    P->wide = fl.wide;
  }
  fl.A = A;
  return TLSAN_OK;
}

// tlsan_index_args.h -- the arguments and host-visible limits of the kernels that pack a batch and build its destination
// index (tlsan_index.h): what the unit that plans the index (tlsan_api_plan.hip) and the sharded step's scans
// (tlsan_api_shard.hip: ScanArgs) need of them.  No kernel.
#pragma once
#include "tlsan_state.h"

struct CountArgs {
  int32_t* n_hot;       // reset here for the scan that follows
  tlsan_batch b;
  int32_t Ls;
  int32_t* cnt_item; int32_t* cnt_user; int32_t* cnt_uc;  // persistent, zero at rest
  // CSEG (many categories): every item use also counts into its item's category -- the category half of its gradient row
  // will sit in that category's segment of Gc, next to the u_cate uses (ApplyArgs.cseg)
  const int32_t* item_cate;
  int32_t cseg;
  int32_t ncate;        // categories (rows of cnt_uc)
  int32_t* flag_user;   // optional: [ceil(U / 256)] set where a user row of that 256-row piece is counted (ScanArgs.flag)
  int32_t skip_users;   // != 0: the user side of the index comes from the counting sort of the batch's user ids (IsortArgs): no counts
};

struct PackArgs {
  tlsan_packed set;
  const int32_t* order;  // sample permutation of the epoch (train.py:191 shuffles the list)
  int32_t lo, Ls, is_test;
  tlsan_batch out;
};

// Which samples share a workgroup of the fused kernel (ScanArgs.bal; one extra block of the index scan's launch).
// The kernel's launch is one workgroup of 16 samples per CU and ends with its slowest workgroup; sample costs are
// heavy-tailed (window length when windows are streamed, session length otherwise).  The batch is ranked by that
// cost (stable counting sort, descending) and dealt out in snake order: round j hands one sample to every group,
// walking the groups forwards on even rounds and backwards on odd ones, so every group gets one sample of each
// sixteenth of the ranking.  perm[16 g + j] = sample j of group g (>= B: none).  A fixed function of the batch.
struct BalArgs {
  const int32_t* sl; const int32_t* sl_new;
  int32_t B, Ls, Sn, by_window;
  int32_t blk;        // index of the block that does this (the first one behind the scan's blocks)
  int32_t* perm;      // NULL: no balancing
};

// the user side from a sort of the batch's ids (usort_block): batches of up to USORT_MAX samples, USORT_NB buckets
#define USORT_MAX 4096
#define USORT_NB 1024
struct UsortArgs {
  const int32_t* u; int32_t B, U;
  int32_t* cur; int32_t* off; int4* urec; int32_t* n_uniq;
  int32_t blk;        // index of the block that does this; u == NULL: none
};

// the item side from a partitioned counting sort (k_isort_*): at most IS_MAXB buckets of at most IS_BSZ ids
#define IS_MAXB 2048
#define IS_BSZ 8192
#define IS_BLK_SLOTS 4096
#define ISORT_MAX_SLOTS (1 << 20)
struct IsortArgs {
  int32_t on;               // 0: the item side is counted per row (k_count)
  tlsan_batch b; int32_t Ls;
  int32_t nbu;              // leading blocks of k_isort_hist that take the samples' single uses (1024 samples each)
  int32_t n, shift, nb;     // rows of the table; nb buckets of 2^shift ids
  int32_t nslots, nblk;     // B * (Ls + Sn + 1) use slots in nblk blocks of IS_BLK_SLOTS
  int32_t* bh;              // [nblk][nb] uses per block and bucket
  int32_t* ids;             // [<= nslots] the valid slots' ids, grouped by bucket
  int32_t* bstart;          // [nb + 1] first position of every bucket
  int32_t* nd;              // [nb] used rows of every bucket
  int4* tmp;                // [<= nslots] records, at the bucket's own positions
  int32_t* cur; int32_t* off; int4* urec; int32_t* n_uniq;
  int32_t* hot_n; int32_t* hot_list;                           // rows with more than AP_HOT uses
  const int32_t* item_cate; int32_t* cnt_uc;                   // category segments: uses counted into the row's category
  int32_t blk, nfin;        // k_index_scan's launch: first finishing block, their number (16 buckets each)
};

struct ScanArgs {
  const int32_t* cnt[3];
  int32_t* off[3];
  int32_t* cur[3];
  int32_t n[3];
  int32_t blk0[3];     // first block of each table in the grid
  int32_t* uniq[3];    // optional: ids with cnt > 0, ascending
  int32_t* n_uniq[3];  // optional: how many
  int4* urec[3];       // optional: (id, first position, count) of the ids with cnt > 0 (lazy L2: rows to update)
  int32_t total[3];    // != 0: off has n+1 entries, off[n] = sum of all counts
  long long* bsum;     // optional [gridDim.x]: per-chunk packed sums (k_scan_block_sums) -- large tables
  int32_t* hot_n[3]; int32_t* hot_list[3];   // optional (with urec): slots of the rows with more than AP_HOT uses
  int32_t sparse;      // bit t set: off / cur of table t are written for the rows with cnt > 0 only -- the user table of a
                       // batch's destination index, which is reached through the batch's ids and the used-row records
                       // only (10 M users: 80 MB of writes per step otherwise; the item offsets are walked per category)
  // optional per table: [ceil(n / 256)] marks of the 256-row pieces that hold a count (set by k_count, cleared here: zero
  // at rest).  A wavefront of either scan kernel covers exactly one piece and skips an unmarked one without reading it:
  // 4096 samples mark at most 4096 pieces of a 10 M-row user table's 39 k (40 MB of counters per pass otherwise)
  int32_t* flag[3];
  int32_t* bs_ticket;   // optional (with bsum): arrival counter of k_scan_block_sums, zero at rest -- its last block scans the sums
  BalArgs bal;         // optional (bal.perm): one more block ranks the batch's samples for the fused kernel's workgroups
  UsortArgs us;        // optional (us.u): one more block builds the user side of the index from a sort of the batch's ids
  IsortArgs is;        // optional (is.on): is.nfin more blocks finish the item side built by the k_isort_* launches
};
#define SCAN_TWO_LEVEL_BLOCKS 16  // tables of more chunks than this take the two-launch form

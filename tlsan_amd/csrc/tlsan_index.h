// tlsan_index.h -- the kernels in front of the fused forward / backward kernel, all launched by tlsan_api.hip alone:
//   k_batch_pack      device-resident batcher
//   k_count           uses per destination row (integer atomics)
//   k_isort_*         the item side of the index from a partitioned counting sort of the batch's ids
//   k_index_scan      exclusive scan of the counts = first sorted position of every row (the fused kernel draws one
//                     position per use from these cursors); its launch also ranks the batch for the fused kernel's
//                     workgroups (balance_block), sorts the user ids (usort_block) and finishes the item sort
//   k_uc_fill         the samples of every category
#pragma once
#include "tlsan_index_args.h"

// Use counts per destination row: one thread per (sample, slot); slots [0,Ls) long positions,
// [Ls,Ls+Sn) session positions, Ls+Sn candidate; the first `nbs` blocks take the samples' single uses instead (user
// row + u_cate row), 256 samples each.
// Category rows find their item-side gradients through the segments of their items (see k_apply),
// so only the u_cate uses are counted per category -- through a histogram in the LDS when the table is small:
// atomics on ONE address execute one after the other (~100 ns each across the XCDs), and with few categories (15 in
// Movies-TV: 273 samples per category) the 4096 u_cate counts alone took 30 us of this kernel's 50.
#define COUNT_LDS_CATES 4096
// one thread per sample (b; nthr threads in the block): the user use and the u_cate use
__device__ __forceinline__ void count_samples_block(const CountArgs& a, int* hist, int b, int nthr) {
  const int B = a.b.B;
  if (b == 0 && a.n_hot) *a.n_hot = 0;
  const bool small = a.ncate <= COUNT_LDS_CATES;
  if (small) {
    for (int c = threadIdx.x; c < a.ncate; c += nthr) hist[c] = 0;
    __syncthreads();
  }
  if (b < B) {
    if (!a.skip_users) {
      atomicAdd(&a.cnt_user[a.b.u[b]], 1);
      if (a.flag_user) a.flag_user[a.b.u[b] >> 8] = 1;
    }
    if (small) atomicAdd(&hist[a.b.u_cate[b]], 1);
    else atomicAdd(&a.cnt_uc[a.b.u_cate[b]], 1);
  }
  if (small) {
    __syncthreads();
    for (int c = threadIdx.x; c < a.ncate; c += nthr)
      if (hist[c] != 0) atomicAdd(&a.cnt_uc[c], hist[c]);
  }
}

__global__ __launch_bounds__(256) void k_count(CountArgs a) {
  __shared__ int hist[COUNT_LDS_CATES];
  const int B = a.b.B, Ls = a.Ls, Sn = a.b.Sn, S = Ls + Sn + 1;
  const int nbs = (B + 255) / 256;
  if ((int)blockIdx.x < nbs) {   // ---- one thread per sample: the user use
    count_samples_block(a, hist, blockIdx.x * 256 + threadIdx.x, 256);
    return;
  }
  const int t = (blockIdx.x - nbs) * 256 + threadIdx.x;
  if (t >= B * S) return;
  const int b = t / S, slot = t - b * S;
  if (slot < Ls) {
    if (slot < min(a.b.sl[b], Ls)) {
      const int id = a.b.hist_i[(size_t)b * Ls + slot];
      atomicAdd(&a.cnt_item[id], 1);
      if (a.cseg) atomicAdd(&a.cnt_uc[a.item_cate[id]], 1);
    }
  } else if (slot < Ls + Sn) {
    const int k = slot - Ls;
    if (k < min(a.b.sl_new[b], Sn)) {
      const int id = a.b.hist_i_new[(size_t)b * Sn + k];
      atomicAdd(&a.cnt_item[id], 1);
      if (a.cseg) atomicAdd(&a.cnt_uc[a.item_cate[id]], 1);
    }
  } else {
    const int id = a.b.i[b];
    atomicAdd(&a.cnt_item[id], 1);
    if (a.cseg) atomicAdd(&a.cnt_uc[a.item_cate[id]], 1);
  }
}

// ------------------------------------------------------------------------------------------
// Device-resident batcher: the reference's DataInput.__next__ / DataInputTest.__next__
// (TLSAN/input.py:17-54, 70-107) over a sample set packed as CSR (tlsan_amd/input.py PackedSet).
// One thread per (sample, slot): slots [0,Ls) the long window -- sl = min(len, Ls), the LAST Ls
// items when the history is longer (input.py:41-45), left-aligned otherwise (:47-49), zeros past
// sl -- slots [Ls, Ls+Sn) the current session padded with zeros, slot Ls+Sn the scalars.
// Samples of every category for the u_cate uses (counting sort by category, after the scan): the
// fused kernel then writes those gradient rows in sample order and draws no cursor for them -- with
// few categories (15 in Movies-TV) 4096 returning atomics on 15 addresses cost it 20 us.
// (the cursor draws of a block's 256 samples go through the LDS as well when the table is small: one returning atomic
//  per block and category instead of one per sample -- 13 -> 4 us with 15 categories)
__global__ __launch_bounds__(256) void k_uc_fill(const int32_t* __restrict__ u_cate, int B, int ncate, int32_t* cur_uc, int32_t* uc_list) {
  __shared__ int hist[COUNT_LDS_CATES];
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (ncate > COUNT_LDS_CATES) {
    if (b < B) uc_list[atomicAdd(&cur_uc[u_cate[b]], 1)] = b;
    return;
  }
  for (int c = threadIdx.x; c < ncate; c += 256) hist[c] = 0;
  __syncthreads();
  const int c = b < B ? u_cate[b] : 0;
  const int rank = b < B ? atomicAdd(&hist[c], 1) : 0;
  __syncthreads();
  for (int k = threadIdx.x; k < ncate; k += 256) {
    const int n = hist[k];
    if (n != 0) hist[k] = atomicAdd(&cur_uc[k], n);   // the block's first position in the category
  }
  __syncthreads();
  if (b < B) uc_list[hist[c] + rank] = b;
}

__global__ void k_batch_pack(PackArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int B = a.out.B, Sn = a.out.Sn, Ls = a.Ls, S = Ls + Sn + 1;
  if (t >= B * S) return;
  const int b = t / S, slot = t - b * S;
  const int smp = a.order[a.lo + b];
  if (slot < Ls) {
    const int h0 = a.set.hist_off[smp], len = a.set.hist_off[smp + 1] - h0;
    const int sl = min(len, Ls), src = h0 + max(len - Ls, 0) + slot;
    const bool v = slot < sl;
    const_cast<int32_t*>(a.out.hist_i)[(size_t)b * Ls + slot] = v ? a.set.hist[src] : 0;
    const_cast<float*>(a.out.hist_t)[(size_t)b * Ls + slot] = v ? a.set.hist_t[src] : 0.0f;
  } else if (slot < Ls + Sn) {
    const int k = slot - Ls;
    const int s0 = a.set.sess_off[smp], n = a.set.sess_off[smp + 1] - s0;
    const_cast<int32_t*>(a.out.hist_i_new)[(size_t)b * Sn + k] = k < n ? a.set.sess[s0 + k] : 0;
  } else {
    const int len = a.set.hist_off[smp + 1] - a.set.hist_off[smp];
    const_cast<int32_t*>(a.out.u)[b] = a.set.u[smp];
    const_cast<int32_t*>(a.out.u_cate)[b] = a.set.cate[smp];
    const_cast<int32_t*>(a.out.sl)[b] = min(len, Ls);                                   // input.py:31
    const_cast<int32_t*>(a.out.sl_new)[b] = a.set.sess_off[smp + 1] - a.set.sess_off[smp];  // :32
    const_cast<int32_t*>(a.out.i)[b] = a.set.target[smp];
    if (a.is_test) const_cast<int32_t*>(a.out.j)[b] = a.set.second[smp];
    else const_cast<float*>(a.out.y)[b] = (float)a.set.second[smp];
  }
}

// Windows in registers (by_window == 0; round 5): a workgroup's time is its longest wavefront's -- session steps in P3,
// window positions in P1 / P5 -- and the launch ends with the workgroups that hold one of the batch's few long sessions
// (25 of 4096 sessions have four or more entries at the bench shape: +1.9 us in P3).  Those workgroups are given short
// WINDOWS to make up for it: samples with sessions of two or more rank first (longest first) and are dealt out in snake
// order as above; the others are ranked by window length, shortest first, and handed out in contiguous runs -- group 0,
// which holds the longest session, gets the shortest windows, the last groups get full windows only (which most
// wavefronts have anyway: half the batch's windows are full).
#define BAL_KEYS 192    // by_window: costs 0 .. 96 (TLSAN_LS_CAP); else 11 * min(session, 15) + window for sessions >= 2, 10 - window below
#define BAL_TAIL_KEY 10 // (by_window == 0) the largest key of a sample with a session of one entry or none

template <int NWV = 16>
__device__ __forceinline__ void balance_block(const BalArgs& b) {   // NWV wavefronts
  constexpr int NT = NWV * 64;
  static_assert(NT >= BAL_KEYS, "a thread per cost");
  __shared__ int wcnt[NWV][BAL_KEYS];  // samples of every cost per wavefront -> where the wavefront's first one of that cost ranks
  __shared__ int start[BAL_KEYS];      // rank of the first sample of every cost
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = b.B, G = (B + 15) / 16;
  const int CH = (B + NT - 1) / NT, nper = 64 * CH;   // wavefront w owns samples [w nper, (w + 1) nper), 64 per round
  for (int o = tid; o < NWV * BAL_KEYS; o += NT) (&wcnt[0][0])[o] = 0;
  __syncthreads();
  auto key_of = [&](int i) {
    if (b.by_window > 0) return min(max(min(b.sl[i], b.Ls), 0), BAL_KEYS - 1);
    const int cs = min(max(min(b.sl_new[i], b.Sn), 0), 15), cl = min(max(min(b.sl[i], b.Ls), 0), 10);
    return cs >= 2 ? 11 * cs + cl : BAL_TAIL_KEY - cl;
  };
  for (int c = 0; c < CH; ++c) {
    const int i = wave * nper + c * 64 + lane;
    if (i < B) atomicAdd(&wcnt[wave][key_of(i)], 1);
  }
  __syncthreads();
  if (tid < BAL_KEYS) {
    int run = 0;
    for (int w = 0; w < NWV; ++w) {
      const int x = wcnt[w][tid];
      wcnt[w][tid] = run;
      run += x;
    }
    start[tid] = run;   // (the cost's total, for the moment)
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = BAL_KEYS - 1; k >= 0; --k) {   // descending: the costliest samples rank first
      const int x = start[k];
      start[k] = run;
      run += x;
    }
  }
  __syncthreads();
  // rounds dealt out in snake order: all of them (by_window), or those that hold the samples with sessions of two or more
  const int n_heavy = b.by_window > 0 ? 16 * G : start[BAL_TAIL_KEY];   // (rank of the first sample of the tail)
  const int H = min(16, (n_heavy + G - 1) / G);
  // (by_window == 0: the groups are numbered backwards -- the full-window groups, the slowest ones now, get the lowest
  //  block numbers and start first; the launch places its workgroups over 0.6 us.  by_window < 0: not, for A/B)
  const bool rev = b.by_window == 0;
  auto place = [&](int rank, int sample) {
    if (rank < H * G) {
      const int j = rank / G, idx = rank - j * G;
      const int g = (j & 1) ? G - 1 - idx : idx;
      b.perm[(rev ? G - 1 - g : g) * 16 + j] = sample;
    } else {   // the tail, shortest windows first: a contiguous run per group
      const int r2 = rank - H * G, per = 16 - H;
      const int g = r2 / per;
      b.perm[(rev ? G - 1 - g : g) * 16 + H + (r2 - g * per)] = sample;
    }
  };
  volatile int* mine = &wcnt[wave][0];   // (wave-private from here on: DS operations of a wavefront execute in order)
  for (int c = 0; c < CH; ++c) {
    const int i = wave * nper + c * 64 + lane;
    const bool v = i < B;
    const int k = v ? key_of(i) : 255;   // (8 bits; the lanes past the batch form a group of their own)
    // lanes of this round with the same cost: eight ballots, one per bit of the cost
    unsigned long long m = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const unsigned long long bb = __ballot((k >> bit) & 1);
      m &= ((k >> bit) & 1) ? bb : ~bb;
    }
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    const int kk = v ? k : 0;
    const int base = start[kk] + mine[kk];                 // ranks taken by earlier wavefronts and earlier rounds
    if (v) place(base + __popcll(below), i);               // within a cost and a round: lane order = sample order
    if (v && below == 0ull) mine[k] = mine[k] + __popcll(m);   // the group's first lane counts the round in
  }
  if (B + tid < 16 * G) place(B + tid, B);   // (a last group that is not full)
}

// ------------------------------------------------------------------------------------------
// The USER side of a batch's destination index without a pass over the user table (one more block of the scan's
// launch): a batch holds B user uses (one per sample), so the used rows, their counts and first positions come from a
// sort of the B ids, B <= USORT_MAX, where the counting form reads (and two scan kernels walk) a counter per table row:
// 10 M users are 2442 of a 10 M + 5 M-row index's 3666 scan blocks.  Writes exactly what the scan writes for a table
// with `sparse` set: cur / off of the used rows, their records (ascending), their number, off[U].
// Round 3 sorted with a bitonic network: 78 barrier-separated phases, ~45 us for ONE block -- and a block that sits on a
// CU that long keeps the fused kernel of the next step, which needs every CU's whole LDS, from placing its last
// workgroup (k_fwd_bwd 45 -> 72 us every other step at 10 M users / 5 M items).  Now a bucket sort in eight phases:
// 1024 buckets of consecutive ids (counted, scanned, filled through LDS cursors), then every id ranks itself inside
// its bucket by counting (smaller ids, and equal ones that came earlier in the bucket) -- a handful of compares per id
// for ids that are spread over the table, O(bucket) each if a batch repeats one user thousands of times.
__device__ __forceinline__ void usort_block(const UsortArgs& a) {   // 1024 threads
  __shared__ int key[USORT_MAX];      // the ids: as they come, later sorted
  __shared__ int srt[USORT_MAX];      // grouped by bucket
  __shared__ int ustart[USORT_MAX];   // bucket counts | cursors, later the first sorted position of every run
  __shared__ int bst[USORT_NB];       // first position of every bucket
  __shared__ int wtot[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int CH = USORT_MAX / 1024;
  int shift = 0;
  while (((a.U - 1) >> shift) >= USORT_NB) ++shift;
  int* bcnt = ustart;                 // [USORT_NB] uses per bucket
  int* bcur = ustart + USORT_NB;      // [USORT_NB] fill cursors
  bcnt[tid] = 0;
  int x[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int i = c * 1024 + tid;
    x[c] = i < a.B ? a.u[i] : -1;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (x[c] >= 0) atomicAdd(&bcnt[x[c] >> shift], 1);
  __syncthreads();
  {   // exclusive scan of the bucket counts (one per thread)
    const int v = bcnt[tid];
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int pre = inc - v;
#pragma unroll
    for (int w = 0; w < 16; ++w) pre += (w < wave) ? wtot[w] : 0;
    bst[tid] = pre;
    bcur[tid] = pre;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (x[c] >= 0) srt[atomicAdd(&bcur[x[c] >> shift], 1)] = x[c];
  __syncthreads();
  // every entry of srt ranks itself inside its bucket
  int dst[CH], val[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int p = c * 1024 + tid;
    dst[c] = -1;
    if (p < a.B) {
      const int v = srt[p], bk = v >> shift, s0 = bst[bk], n = bcnt[bk];
      int rank = 0;
      for (int j = s0; j < s0 + n; ++j) {
        const int y = srt[j];
        rank += (y < v || (y == v && j < p)) ? 1 : 0;
      }
      dst[c] = s0 + rank;
      val[c] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (dst[c] >= 0) key[dst[c]] = val[c];
  __syncthreads();
  // runs of equal ids: a thread takes CH consecutive sorted entries
  const int i0 = tid * CH;
  int mine = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int i = i0 + c;
    mine += (i < a.B && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
  }
  int inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int j = inc - mine, nu = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    j += (w < wave) ? wtot[w] : 0;
    nu += wtot[w];
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int i = i0 + c;
    if (i < a.B && (i == 0 || key[i] != key[i - 1])) ustart[j++] = i;
  }
  __syncthreads();
  for (int r = tid; r < nu; r += 1024) {
    const int st = ustart[r], row = key[st], cnt = (r + 1 < nu ? ustart[r + 1] : a.B) - st;
    a.urec[r] = make_int4(row, st, cnt, 0);
    a.cur[row] = st;
    a.off[row] = st;
  }
  if (tid == 0) {
    *a.n_uniq = nu;
    a.off[a.U] = a.B;
  }
}

// ------------------------------------------------------------------------------------------
// The ITEM side of a batch's destination index without a counter per table row (round 4): a partitioned counting sort of
// the batch's item uses (window, session, candidate).  With millions of items the counting form costs a global atomic
// per use on a table that does not fit the caches and two passes over every counter (k_scan_block_sums + k_index_scan:
// 16 + 41 us for 5 M items on an otherwise idle GPU); here the work is proportional to the batch.  The ids are split
// into buckets of 2^shift consecutive ids (at most IS_MAXB buckets of at most IS_BSZ ids: tables up to 16 M rows), and a
// bucket's counters live in the LDS:
//   k_isort_hist      blocks of IS_BLK_SLOTS use slots: LDS histogram over the buckets -> one row of `bh` per block
//                     (its leading blocks take the samples' single uses, as k_count's do)
//   k_isort_scatter   same blocks: a bucket's first position = uses of lower buckets + this bucket's uses in earlier
//                     blocks (column sums of bh, read by every block from the L2); ids scattered into their bucket's
//                     range of `ids` (order inside a bucket: whatever the LDS atomics give -- it does not matter)
//   k_isort_bucket    one block per bucket: counts of its ids in the LDS, scanned -> for every used id its first sorted
//                     position (cur / off, written for used rows only) and its record (id, first, uses) at the
//                     bucket's own range of `tmp`; category segments: uses added to the id's category counter, one
//                     atomic per used ROW instead of one per use
//   isort_finish      (blocks of k_index_scan's launch, beside the category scan) records compacted into urec in id
//                     order, hot rows listed, n_uniq, off[I]
// Writes what the scan writes for a table with `sparse` set -- a fixed function of the batch (records ascending by id;
// the hot list's order is the atomics', as before).  Consumers must reach off / cur through ids or records only: the
// lazy-L2 SGD step with category segments (tlsan_api.hip: build_index).
// item id of use slot t (k_count's enumeration: sample-major; long positions, session positions, the candidate), -1: padding
__device__ __forceinline__ int isort_slot_id(const IsortArgs& a, int t) {
  if (t >= a.nslots) return -1;
  const tlsan_batch& b = a.b;
  const int Ls = a.Ls, Sn = b.Sn, S = Ls + Sn + 1;
  const int smp = t / S, slot = t - smp * S;
  if (slot < Ls) return slot < min(b.sl[smp], Ls) ? b.hist_i[(size_t)smp * Ls + slot] : -1;
  if (slot < Ls + Sn) return (slot - Ls) < min(b.sl_new[smp], Sn) ? b.hist_i_new[(size_t)smp * Sn + (slot - Ls)] : -1;
  return b.i[smp];
}
#define IS_PT (IS_BLK_SLOTS / 1024)   // slots per thread

__global__ __launch_bounds__(1024) void k_isort_hist(IsortArgs a, CountArgs ca) {
  __shared__ int h[COUNT_LDS_CATES > IS_MAXB ? COUNT_LDS_CATES : IS_MAXB];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < a.nbu) {     // the samples' single uses (u_cate row; user row unless sorted)
    count_samples_block(ca, h, blockIdx.x * 1024 + tid, 1024);
    return;
  }
  const int blk = (int)blockIdx.x - a.nbu;
  h[tid] = 0;
  h[tid + 1024] = 0;
  __syncthreads();
  int id[IS_PT];
#pragma unroll
  for (int k = 0; k < IS_PT; ++k) id[k] = isort_slot_id(a, blk * IS_BLK_SLOTS + k * 1024 + tid);
#pragma unroll
  for (int k = 0; k < IS_PT; ++k)
    if (id[k] >= 0) atomicAdd(&h[id[k] >> a.shift], 1);
  __syncthreads();
  for (int c = tid; c < a.nb; c += 1024) a.bh[(size_t)blk * a.nb + c] = h[c];
}

__global__ __launch_bounds__(1024) void k_isort_scatter(IsortArgs a) {
  __shared__ int base[IS_MAXB];
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x;
  // the ids first: their loads fly while the column sums are formed
  int id[IS_PT];
#pragma unroll
  for (int k = 0; k < IS_PT; ++k) id[k] = isort_slot_id(a, blk * IS_BLK_SLOTS + k * 1024 + tid);
  // thread t owns buckets 2t and 2t + 1 (consecutive: the exclusive scan over the threads' pairs is the scan over buckets)
  int below[2] = {0, 0}, total[2] = {0, 0};
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int c = 2 * tid + e;
    if (c < a.nb) {
      const int32_t* col = a.bh + c;
      for (int j0 = 0; j0 < a.nblk; j0 += 8) {   // 8 loads in flight
        int v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(size_t)min(j0 + u, a.nblk - 1) * a.nb];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int xx = (j0 + u < a.nblk) ? v[u] : 0;
          total[e] += xx;
          below[e] += (j0 + u < blk) ? xx : 0;
        }
      }
    }
  }
  const int tsum = total[0] + total[1];
  int inc = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int start = inc - tsum;
#pragma unroll
  for (int w = 0; w < 16; ++w) start += (w < wave) ? wsum[w] : 0;
  base[2 * tid] = start + below[0];
  base[2 * tid + 1] = start + total[0] + below[1];
  if (blk == 0) {
    if (2 * tid < a.nb) a.bstart[2 * tid] = start;
    if (2 * tid + 1 < a.nb) a.bstart[2 * tid + 1] = start + total[0];
    if (2 * tid == a.nb - 1 || 2 * tid + 1 == a.nb - 1) a.bstart[a.nb] = start + tsum;   // (the last bucket's owner: nothing lies behind it)
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < IS_PT; ++k)
    if (id[k] >= 0) a.ids[atomicAdd(&base[id[k] >> a.shift], 1)] = id[k];
}

// (its FIRST block, when us.u is set, is the user side's sort: independent of everything here and the longest block of
//  the launch -- dispatched first it runs beside the bucket blocks; inside k_index_scan's launch it was the long pole)
__global__ __launch_bounds__(1024) void k_isort_bucket(IsortArgs a, UsortArgs us) {
  const int ub = us.u != nullptr ? 1 : 0;
  if (ub && blockIdx.x == 0) {
    usort_block(us);
    return;
  }
  __shared__ int h[IS_BSZ];
  __shared__ long long wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = (int)blockIdx.x - ub;
  const int lo = a.bstart[b], n = a.bstart[b + 1] - lo;
  if (n == 0) {   // (block-uniform)
    if (tid == 0) a.nd[b] = 0;
    return;
  }
  const int id0 = b << a.shift;
  constexpr int PER = IS_BSZ / 1024;
#pragma unroll
  for (int e = 0; e < PER; ++e) h[e * 1024 + tid] = 0;
  __syncthreads();
  for (int j = tid; j < n; j += 1024) atomicAdd(&h[a.ids[lo + j] - id0], 1);
  __syncthreads();
  int c[PER];
  long long tsum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    c[k] = h[tid * PER + k];
    tsum += (long long)c[k] + ((long long)(c[k] > 0) << 32);
  }
  long long inc = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  long long run = inc - tsum;
#pragma unroll
  for (int w = 0; w < 16; ++w) run += (w < wave) ? wsum[w] : 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (c[k] > 0) {
      const int id = id0 + tid * PER + k, first = lo + (int)(run & 0xffffffffLL);
      a.cur[id] = first;
      a.off[id] = first;
      a.tmp[lo + (int)(run >> 32)] = make_int4(id, first, c[k], 0);
      if (a.cnt_uc != nullptr) atomicAdd(&a.cnt_uc[a.item_cate[id]], c[k]);
      run += (long long)c[k] + (1LL << 32);
    }
  }
  if (tid == 1023) a.nd[b] = (int)(run >> 32);
}

// one finishing block (k_index_scan's launch): 16 buckets, one per wavefront -- records to their place in urec
__device__ __forceinline__ void isort_finish_block(const IsortArgs& a, int j) {
  __shared__ int dbase[IS_MAXB];
  __shared__ int wtot[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v0 = 2 * tid < a.nb ? a.nd[2 * tid] : 0, v1 = 2 * tid + 1 < a.nb ? a.nd[2 * tid + 1] : 0;
  int inc = v0 + v1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int pre = inc - (v0 + v1), nu = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    pre += (w < wave) ? wtot[w] : 0;
    nu += wtot[w];
  }
  dbase[2 * tid] = pre;
  dbase[2 * tid + 1] = pre + v0;
  __syncthreads();
  const int bb = j * 16 + wave;
  if (bb < a.nb) {
    const int n = a.nd[bb], d0 = dbase[bb];
    const int4* src = a.tmp + a.bstart[bb];
    for (int r = lane; r < n; r += 64) {
      const int4 rec = src[r];
      a.urec[d0 + r] = rec;
      if (rec.z > AP_HOT) {
        const int hh = atomicAdd(a.hot_n, 1);
        if (hh < AP_HOT_CAP) a.hot_list[hh] = d0 + r;
      }
    }
  }
  if (j == 0 && tid == 0) {
    *a.n_uniq = nu;
    a.off[a.n] = a.bstart[a.nb];
  }
}


// Exclusive scan of the per-row counts, one launch: block j of a table owns ids
// [4096 j, 4096 j + 4096); it first sums every count that precedes its chunk (coalesced
// re-read of at most n ints from L2: cheaper than a second launch or a serial carry chain),
// then scans its own chunk.  The number of non-zero counts is scanned alongside (high 32 bits
// of a packed 64-bit sum) to compact the list of used rows.
// The re-read is quadratic in the number of chunks, so for large tables (millions of rows) a
// first launch leaves one packed sum per chunk (k_scan_block_sums) and the blocks add up the
// preceding CHUNK sums instead (ScanArgs.bsum).
__global__ __launch_bounds__(1024) void k_scan_block_sums(ScanArgs a) {
  __shared__ long long wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int which = 0;
  if ((int)blockIdx.x >= a.blk0[1]) which = 1;
  if ((int)blockIdx.x >= a.blk0[2]) which = 2;
  const int32_t* __restrict__ cnt = a.cnt[which];
  const int n = a.n[which];
  const int i0 = ((int)blockIdx.x - a.blk0[which]) * 4096 + tid * 4;
  long long part = 0;
  int c4[4] = {0, 0, 0, 0};
  const bool marked = a.flag[which] == nullptr || i0 >= n || a.flag[which][i0 >> 8] != 0;   // (wave-uniform)
  if (!marked) {
  } else if (i0 + 3 < n) {               // (chunks start at multiples of 4096: 16-byte aligned)
    const int4 v = *(const int4*)(cnt + i0);
    c4[0] = v.x; c4[1] = v.y; c4[2] = v.z; c4[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) c4[k] = (i0 + k < n) ? cnt[i0 + k] : 0;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) part += (long long)c4[k] + ((long long)(c4[k] > 0) << 32);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) wsum[wave] = part;
  __syncthreads();
  __shared__ int s_last;
  if (tid == 0) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += wsum[w];
    if (a.bs_ticket == nullptr) {
      a.bsum[blockIdx.x] = t;
    } else {   // published with a returning atomic: the last block to arrive reads every sum with device-scope loads
      const unsigned long long old = atomicExch((unsigned long long*)&a.bsum[blockIdx.x], (unsigned long long)t);
      asm volatile("" ::"v"(old));
      s_last = atomicAdd(a.bs_ticket, 1) == (int)gridDim.x - 1;
    }
  }
  if (a.bs_ticket == nullptr) return;
  __syncthreads();
  if (!s_last) return;
  // ---- the last block: the sums of every table's chunks -> exclusive prefixes, in place (k_index_scan then reads ONE
  // value per block where every block used to add up all the sums before its own: 3663 chunks of a 10 M + 5 M-row index,
  // 54 MB of reads)
  __shared__ long long carry;
  for (int t = 0; t < 3; ++t) {
    const int b0 = a.blk0[t], b1 = t < 2 ? a.blk0[t + 1] : (int)gridDim.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int k0 = b0; k0 < b1; k0 += 1024) {
      const int k = k0 + tid;
      const long long v = k < b1 ? __hip_atomic_load(&a.bsum[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
      long long inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const long long x = __shfl_up(inc, o);
        if (lane >= o) inc += x;
      }
      if (lane == 63) wsum[wave] = inc;
      __syncthreads();
      long long pre = carry + inc - v;
#pragma unroll
      for (int w = 0; w < 16; ++w) pre += (w < wave) ? wsum[w] : 0;
      if (k < b1) a.bsum[k] = pre;
      __syncthreads();
      if (tid == 1023) carry = pre + v;
      __syncthreads();
    }
  }
  if (tid == 0) *a.bs_ticket = 0;   // zero at rest
}

// one scan block of NT threads: chunk `blk` of its table, 4 NT consecutive counts.  (Round 6 also ran the scan of cache-resident
// tables as 256-thread workgroups over chunks of 1024 counts, so that its blocks find a slot beside the row-sum workgroups:
// the kernel itself 16 -> 28 us beside the step, the step equal or 1-2 us slower -- profiles/r06_ab_scan_small.txt; removed.)
template <int NT>
__device__ __forceinline__ void index_scan_block(const ScanArgs& a, int blk) {
  constexpr int CHK = 4 * NT;
  __shared__ long long wsum[NT / 64];
  __shared__ long long prefix;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int which = 0;
  if (blk >= a.blk0[1]) which = 1;
  if (blk >= a.blk0[2]) which = 2;
  const int32_t* __restrict__ cnt = a.cnt[which];
  const int n = a.n[which];
  const int base = (blk - a.blk0[which]) * CHK;
  auto pack = [](int c) { return (long long)c + ((long long)(c > 0) << 32); };
  // ---- packed sum over cnt[0, base)
  long long part = 0;
  if (a.bsum != nullptr && a.bs_ticket != nullptr) {
    part = tid == 0 ? a.bsum[blk] : 0;   // (k_scan_block_sums left the exclusive prefix of this block's table)
  } else if (a.bsum != nullptr) {
    for (int k = a.blk0[which] + tid; k < blk; k += NT) part += a.bsum[k];
  } else {
    for (int k = tid * 4; k < base; k += CHK) {
      const int4 v = *(const int4*)(cnt + k);  // base is a multiple of the chunk -> always in range
      part += pack(v.x) + pack(v.y) + pack(v.z) + pack(v.w);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) wsum[wave] = part;
  __syncthreads();
  if (tid == 0) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += wsum[w];
    prefix = t;
  }
  __syncthreads();
  const long long pre = prefix;
  __syncthreads();
  // ---- own chunk
  const int i0 = base + tid * 4;
  int v[4] = {0, 0, 0, 0};
  const bool full = i0 + 3 < n;          // (chunks start at multiples of 4 NT: 16-byte accesses)
  const bool marked = a.flag[which] == nullptr || i0 >= n || a.flag[which][i0 >> 8] != 0;   // (wave-uniform: a wavefront = one 256-row piece)
  if (!marked) {
  } else if (full) {
    const int4 t = *(const int4*)(cnt + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (i0 + k < n) ? cnt[i0 + k] : 0;
  }
  const long long tsum = pack(v[0]) + pack(v[1]) + pack(v[2]) + pack(v[3]);
  long long inc = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  long long run = pre + inc - tsum;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) run += (w < wave) ? wsum[w] : 0;
  int32_t* off = a.off[which];
  int32_t* cur = a.cur[which];
  int32_t* uniq = a.uniq[which];
  int4* urec = a.urec[which];
  const bool dense4 = full && !((a.sparse >> which) & 1);   // the four offsets as one 16-byte store each
  if (dense4) {
    const int o0 = (int)(run & 0xffffffffLL);
    const int4 o4 = make_int4(o0, o0 + v[0], o0 + v[0] + v[1], o0 + v[0] + v[1] + v[2]);
    *(int4*)(off + i0) = o4;
    if (cur) *(int4*)(cur + i0) = o4;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) {
      const int o = (int)(run & 0xffffffffLL);
      if (!dense4 && (!((a.sparse >> which) & 1) || v[k] > 0)) {
        off[i0 + k] = o;
        if (cur) cur[i0 + k] = o;
      }
      if (uniq && v[k] > 0) uniq[(int)(run >> 32)] = i0 + k;
      if (urec && v[k] > 0) urec[(int)(run >> 32)] = make_int4(i0 + k, o, v[k], 0);
      if (urec && a.hot_n[which] && v[k] > AP_HOT) {
        const int h = atomicAdd(a.hot_n[which], 1);
        if (h < AP_HOT_CAP) a.hot_list[which][h] = (int)(run >> 32);
      }
      run += pack(v[k]);
      if (i0 + k == n - 1) {
        if (a.n_uniq[which]) *a.n_uniq[which] = (int)(run >> 32);
        if (a.total[which]) off[n] = (int)(run & 0xffffffffLL);
      }
    }
  }
  if (a.flag[which] != nullptr && marked && lane == 0 && i0 < n) a.flag[which][i0 >> 8] = 0;   // zero at rest
}

__global__ __launch_bounds__(1024) void k_index_scan(ScanArgs a) {
  if (a.bal.perm != nullptr && (int)blockIdx.x == a.bal.blk) {
    balance_block<16>(a.bal);
    return;
  }
  if (a.us.u != nullptr && (int)blockIdx.x == a.us.blk) {
    usort_block(a.us);
    return;
  }
  if (a.is.on != 0 && (int)blockIdx.x >= a.is.blk) {
    isort_finish_block(a.is, (int)blockIdx.x - a.is.blk);
    return;
  }
  index_scan_block<1024>(a, blockIdx.x);
}

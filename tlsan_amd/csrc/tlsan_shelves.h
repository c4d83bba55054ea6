// tlsan_shelves.h -- category shelves: for each row the S lists (categories of an index, tlsan_lists.h) whose m-lists rank
// highest, with those m-lists, in one scan of the index.  Never a [B, I] score array, never a [B, nlists, m] array.
//
// L(b, c): the m best eligible items of list c for row b -- tlsan_eval_topk_lists' list of a row that probes c alone, ids
// and score bits (the scores are lists_scan's: score_tiles4<D, false> on the same operands, ListScore / eval_score; the
// selection is TopkSmem's, whose result is the m largest keys whatever the order of the offers).  n(b, c): its valid
// entries.  List c is a CANDIDATE of row b when no entry of skip[b, :] names it and n(b, c) >= min_items; its rank key is
// the 64-bit key of entry rank_at < min_items of L(b, c).  Candidate x comes before candidate y when its rank key is
// larger, or equal with the lower list id (shelf_before): a total order, so the S first candidates are a function of
// (row, index, arguments) alone, whatever the plan.
//
// The PLAN (host-built, from the index's list lengths) splits the non-empty lists into
//   segments  seg_lists[seg_off[s] .. seg_off[s + 1]): lists no longer than the caller's threshold, packed in list order;
//   big lists big_off[j] .. big_off[j + 1] of the slices big_slices[t] = (list, lo, hi): positions lo .. hi of the list,
//             at most SHELF_SLICES_MAX slices a list.
// k_shelves_scan, grid (ceil(B / 16), nseg + nbs): a segment's workgroup walks its lists one after another -- the tile
// loop into a TopkSmem with K = m, topk_reselect, the offer of the list's m keys to the rows' shelf tables in LDS (S
// slots of m keys and the list id per row, unordered: a full table replaces its last candidate in shelf_before's order),
// the selection state set back -- and writes its tables to [B, nseg, S] slots; a slice's workgroup writes the m keys of its
// positions to [B, nbs, m].  k_shelves_merge, one wavefront per row: the slices of a big list folded into its m best (the
// slices hold disjoint positions), tested as a candidate; every candidate offered to one table; the table sorted and
// written out.  Every id the plan holds is checked before it addresses anything (a list id against nlists, positions
// against the list's length), so a wrong plan costs shelves, never a read outside the index.
//
// The tile loop is the FOURTH copy of topk_scan's (tlsan_topk.h says why k_eval_topk keeps its text; lists_scan is the
// third): its rows are 16 consecutive rows as topk_scan's, its item mapping lists_scan's ListMap, and it runs inside a
// loop over lists.  A fix to the scan's prologue, tile loop or offer loop goes into all four.
#pragma once
#include "tlsan_lists.h"

#define SHELF_SMAX 32          // most shelves of a row
#define SHELF_MMAX 64          // most items of a shelf
#define SHELF_SKIP_MAX 8       // most skipped lists of a row
#define SHELF_SLICES_MAX 16    // most slices of a big list

struct ShelvesArgs {
  TopkArgs t;                  // e, K = m, the exclusion lists (ids / scores unused)
  const int32_t* list_off;     // [nlists + 1]
  const int32_t* list_items;
  int32_t nlists;
  int32_t S, min_items, rank_at;
  const int32_t* seg_off;      // [nseg + 1] into seg_lists
  const int32_t* seg_lists;    // [nsmall] list ids
  const int32_t* big_off;      // [nbig + 1] into big_slices
  const int32_t* big_slices;   // [nbs, 3] (list, lo, hi)
  int32_t nseg, nsmall, nbig, nbs;
  const int32_t* skip;         // [B, X] or NULL
  int32_t X;
  topk_key_t* seg_keys;        // [B, nseg, S, m]
  int32_t* seg_cat;            // [B, nseg, S] (-1: no candidate)
  topk_key_t* big_keys;        // [B, nbs, m]
  int32_t* cats;               // [B, S]
  int32_t* ids;                // [B, S, m]
  float* scores;               // [B, S, m]
};

// candidate (ka, ca) comes before candidate (kb, cb)
__device__ __forceinline__ bool shelf_before(topk_key_t ka, int ca, topk_key_t kb, int cb) { return ka > kb || (ka == kb && ca < cb); }

// The shelf tables of a workgroup's rows: S slots of m keys each (slot e of row u at keys[u][e * m ..]), unordered.
template <int ROWS>
struct ShelfTable {
  topk_key_t keys[ROWS][SHELF_SMAX * 8];   // S * m <= 256 keys a row
  int cat[ROWS][SHELF_SMAX];
  int n[ROWS];
  int dst[ROWS];                           // where the row's current candidate goes (-1: nowhere)
  int skip[ROWS][SHELF_SKIP_MAX];
};

// The slot row u's candidate (rank key rk, list c) takes in its table, -1 when S candidates come before it (one thread a row).
template <int ROWS>
__device__ __forceinline__ int shelf_slot(ShelfTable<ROWS>& tb, int u, int S, int m, int rank_at, topk_key_t rk, int c) {
  const int n = tb.n[u];
  if (n < S) {
    tb.n[u] = n + 1;
    return n;
  }
  int w = 0;
  topk_key_t wk = tb.keys[u][rank_at];
  int wc = tb.cat[u][0];
  for (int e = 1; e < S; ++e) {              // the table's last candidate
    const topk_key_t k = tb.keys[u][e * m + rank_at];
    const int cc = tb.cat[u][e];
    if (shelf_before(wk, wc, k, cc)) { w = e; wk = k; wc = cc; }
  }
  return shelf_before(rk, c, wk, wc) ? w : -1;
}

template <int ROWS>
__device__ __forceinline__ bool shelf_skipped(const ShelfTable<ROWS>& tb, int u, int X, int c) {
  bool hit = false;
  for (int x = 0; x < X; ++x) hit |= tb.skip[u][x] == c;
  return hit;
}

// A workgroup of grid (ceil(B / 16), nseg + nbs): unit y < nseg is segment y, else slice y - nseg.
template <int D, int KP, int BUF>
__device__ __forceinline__ void shelves_scan(TopkSmem<KP, BUF>& sm, ShelfTable<16>& tb, const ShelvesArgs& sa) {
  const TopkArgs& ta = sa.t;
  const EvalArgs& a = ta.e;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int u0 = blockIdx.x * 16;
  const int y = blockIdx.y, m = ta.K, S = sa.S;
  const bool seg = y < sa.nseg;
  int l0, l1;                                // the unit's lists: positions of seg_lists, or the one slice
  if (seg) {
    l0 = min(max(sa.seg_off[y], 0), sa.nsmall);
    l1 = min(max(sa.seg_off[y + 1], l0), sa.nsmall);
  } else {
    l0 = y - sa.nseg;
    l1 = l0 + 1;
  }
  ListScore pol(a);
  f32x4 af[D / 16];
  load_user_frag<D>(a, u0, q, r, af);
  bool uv[4];
  int xlo[4], xhi[4];
  topk_key_t thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = u0 + 4 * q + i;
    uv[i] = pol.row(i, u);
    xlo[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u] : 0;
    xhi[i] = (uv[i] && ta.excl_off) ? ta.excl_off[u + 1] : 0;
  }
  if (threadIdx.x < 16) tb.n[threadIdx.x] = 0;
  if (threadIdx.x < 16 * SHELF_SKIP_MAX) {
    const int u = threadIdx.x / SHELF_SKIP_MAX, x = threadIdx.x % SHELF_SKIP_MAX;
    tb.skip[u][x] = (sa.skip && x < sa.X && u0 + u < a.B) ? sa.skip[(size_t)(u0 + u) * sa.X + x] : -1;
  }
  for (int li = l0; li < l1; ++li) {
    const int c = seg ? sa.seg_lists[li] : sa.big_slices[3 * li];
    if ((unsigned)c >= (unsigned)sa.nlists) continue;            // (uniform)
    int base = sa.list_off[c];
    int cnt = sa.list_off[c + 1] - base;
    if (!seg) {
      const int lo = min(max(sa.big_slices[3 * li + 1], 0), max(cnt, 0));
      const int hi = min(max(sa.big_slices[3 * li + 2], lo), max(cnt, 0));
      base += lo;
      cnt = hi - lo;
    }
    if (cnt <= 0) continue;                                       // (uniform)
    const ListMap map(sa.list_items + base, cnt, a.I);
    topk_init(sm);
#pragma unroll
    for (int i = 0; i < 4; ++i) thr[i] = 0ull;
    __syncthreads();
    const int step = 256;
    const int nround = (cnt + step - 1) / step;
    const int w0 = wave * 64;
    auto locals = [&](int n0, int (&loc)[4]) {
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) loc[tt] = map.local(min(n0 + 16 * tt + r, cnt - 1));
    };
    int nxt[4] = {0, 0, 0, 0};   // the coming round's
    if (w0 < cnt) locals(w0, nxt);
    int ph = 0;
    for (int rd = 0; rd < nround; ++rd) {
      const int n0 = rd * step + w0;
      topk_key_t key[16];
      unsigned pend = 0;
      if (n0 < cnt) {
        int item[4];
        bool held[4];
        f32x4 acc[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          held[tt] = map.holds(nxt[tt]);
          item[tt] = held[tt] ? nxt[tt] : 0;
        }
        if (n0 < cnt - step) locals(n0 + step, nxt);
        score_tiles4<D, false>(a, af, item, q, acc);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
          const bool vn = n0 + 16 * tt + r < cnt && held[tt];
          const int gn = item[tt] * a.id_mul + a.id_add;  // global item id
          pol.col(acc[tt], item[tt]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            key[4 * tt + i] = topk_key(pol.score(i), gn);
            // (the exclusion list is searched only for scores that pass the threshold)
            if (vn && uv[i] && pol.may(i, gn) && key[4 * tt + i] > thr[i] && !topk_in_list(ta.excl_ids, xlo[i], xhi[i], gn))
              pend |= 1u << (4 * tt + i);
          }
        }
      }
      topk_offer(sm, key, pend, 4 * q, thr, m, ph);
    }
    bool left = false;
#pragma unroll
    for (int u = 0; u < 16; ++u) left |= sm.cnt[u] != 0;
    if (left) topk_reselect(sm);
    if (!seg) {                                                   // a slice: its m keys, whatever they are
      for (int p = threadIdx.x; p < 16 * m; p += 256) {
        const int u = p / m, j = p % m;
        if (u0 + u < a.B) sa.big_keys[((size_t)(u0 + u) * sa.nbs + li) * m + j] = sm.kept[u][j];
      }
      return;
    }
    if (threadIdx.x < 16) {
      const int u = threadIdx.x;
      const bool cand = sm.kept[u][sa.min_items - 1] != 0ull && !shelf_skipped(tb, u, sa.X, c);
      const int d = cand ? shelf_slot(tb, u, S, m, sa.rank_at, sm.kept[u][sa.rank_at], c) : -1;
      tb.dst[u] = d;
      if (d >= 0) tb.cat[u][d] = c;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < 16 * m; p += 256) {
      const int u = p / m, j = p % m;
      const int d = tb.dst[u];
      if (d >= 0) tb.keys[u][d * m + j] = sm.kept[u][j];
    }
    __syncthreads();
  }
  if (!seg) {                                                     // a slice that held nothing
    for (int p = threadIdx.x; p < 16 * m; p += 256) {
      const int u = p / m, j = p % m;
      if (u0 + u < a.B) sa.big_keys[((size_t)(u0 + u) * sa.nbs + l0) * m + j] = 0ull;
    }
    return;
  }
  __syncthreads();
  for (int p = threadIdx.x; p < 16 * S * m; p += 256) {
    const int u = p / (S * m), e = (p % (S * m)) / m;
    if (u0 + u >= a.B) continue;
    const size_t o = ((size_t)(u0 + u) * sa.nseg + y) * S * m + p % (S * m);
    sa.seg_keys[o] = e < tb.n[u] ? tb.keys[u][p % (S * m)] : 0ull;
  }
  for (int p = threadIdx.x; p < 16 * S; p += 256) {
    const int u = p / S, e = p % S;
    if (u0 + u < a.B) sa.seg_cat[((size_t)(u0 + u) * sa.nseg + y) * S + e] = e < tb.n[u] ? tb.cat[u][e] : -1;
  }
}

// (d = 256: one workgroup a CU by registers.  Under (256, 2), where k_lists_topk<256> sits at 242 to 256 VGPRs, the state
//  carried over the loop of lists -- the unit's bounds, the table's arguments -- spilled 14 VGPRs to scratch.)
template <int D, int KP, int BUF>
__global__ __launch_bounds__(256, D == 256 ? 1 : 2) void k_shelves_scan(ShelvesArgs sa) {
  __shared__ TopkSmem<KP, BUF> sm;
  __shared__ ShelfTable<16> tb;
  shelves_scan<D, KP, BUF>(sm, tb, sa);
}

// One wavefront per row: the row's candidates -- its segments' tables and its big lists -- into one table, sorted, written.
__global__ __launch_bounds__(64) void k_shelves_merge(ShelvesArgs sa) {
  __shared__ ShelfTable<1> tb;
  __shared__ topk_key_t bk[SHELF_SLICES_MAX * SHELF_MMAX];
  __shared__ topk_key_t bsel[SHELF_MMAX];
  __shared__ int order[SHELF_SMAX];
  const int row = blockIdx.x, t = threadIdx.x;
  const int m = sa.t.K, S = sa.S;
  if (t == 0) tb.n[0] = 0;
  if (t < SHELF_SKIP_MAX) tb.skip[0][t] = (sa.skip && t < sa.X) ? sa.skip[(size_t)row * sa.X + t] : -1;
  __syncthreads();
  // the segments' candidates (already tested)
  const int nsc = sa.nseg * S;
  for (int e = 0; e < nsc; ++e) {
    const int c = sa.seg_cat[(size_t)row * nsc + e];
    if (c < 0) continue;                                          // (uniform)
    const topk_key_t* src = sa.seg_keys + ((size_t)row * nsc + e) * m;
    if (t == 0) tb.dst[0] = shelf_slot(tb, 0, S, m, sa.rank_at, src[sa.rank_at], c);
    __syncthreads();
    const int d = tb.dst[0];
    if (d >= 0) {
      if (t < m) tb.keys[0][d * m + t] = src[t];
      if (t == 0) tb.cat[0][d] = c;
    }
    __syncthreads();
  }
  // the big lists: the m best of a list's slices, then the candidate's test
  for (int j = 0; j < sa.nbig; ++j) {
    const int t0 = min(max(sa.big_off[j], 0), sa.nbs);
    const int t1 = min(max(sa.big_off[j + 1], t0), min(sa.nbs, t0 + SHELF_SLICES_MAX));
    if (t1 <= t0) continue;
    const int c = sa.big_slices[3 * t0];
    if ((unsigned)c >= (unsigned)sa.nlists) continue;
    const int n = (t1 - t0) * m;
    for (int p = t; p < n; p += 64) bk[p] = sa.big_keys[((size_t)row * sa.nbs + t0) * m + p];
    if (t < m) bsel[t] = 0ull;
    __syncthreads();
    for (int p = t; p < n; p += 64) {
      const topk_key_t k = bk[p];
      if (k == 0ull) continue;
      int rk = 0;
      for (int o = 0; o < n; ++o) rk += (bk[o] > k || (bk[o] == k && o < p)) ? 1 : 0;
      if (rk < m) bsel[rk] = k;
    }
    __syncthreads();
    if (t == 0) {
      const bool cand = bsel[sa.min_items - 1] != 0ull && !shelf_skipped(tb, 0, sa.X, c);
      tb.dst[0] = cand ? shelf_slot(tb, 0, S, m, sa.rank_at, bsel[sa.rank_at], c) : -1;
    }
    __syncthreads();
    const int d = tb.dst[0];
    if (d >= 0) {
      if (t < m) tb.keys[0][d * m + t] = bsel[t];
      if (t == 0) tb.cat[0][d] = c;
    }
    __syncthreads();
  }
  // the table in shelf_before's order (equal candidates, which no plan of distinct lists holds: the lower slot first)
  const int n = tb.n[0];
  if (t < n) {
    const topk_key_t k = tb.keys[0][t * m + sa.rank_at];
    const int c = tb.cat[0][t];
    int pos = 0;
    for (int e = 0; e < n; ++e) {
      const topk_key_t ke = tb.keys[0][e * m + sa.rank_at];
      const int ce = tb.cat[0][e];
      pos += (shelf_before(ke, ce, k, c) || (ke == k && ce == c && e < t)) ? 1 : 0;
    }
    order[pos] = t;
  }
  __syncthreads();
  for (int p = t; p < S * m; p += 64) {
    const int sh = p / m, j = p % m;
    const topk_key_t key = sh < n ? tb.keys[0][order[sh] * m + j] : 0ull;
    const size_t o = (size_t)row * S * m + p;
    sa.ids[o] = topk_key_id(key);
    sa.scores[o] = topk_key_score(key);
  }
  if (t < S) sa.cats[(size_t)row * S + t] = t < n ? tb.cat[0][order[t]] : -1;
}

// tlsan_attn_lds.h -- the layout of k_fwd_bwd's dynamic LDS block: the variant predicates that decide it, every region's
// offset and size, and the bytes a launch asks for.  The kernel (tlsan_attn.h) forms its pointers from it, the launcher
// (tlsan_attn_inst.h) takes its byte count from it, tests/attn_lds_dump.hip prints it on the host (tests/test_attn_lds_cpu.py).
// Needs Geo and the TLSAN_* caps only.  One list of regions, laid out from two kinds of base: the kernel gives it the
// block's float* and gets its pointers; the host gives it the dword offset 0 and gets offsets.  Sizes are in dwords.
#pragma once
#include <type_traits>
#include "tlsan_common.h"

#ifndef TLSAN_STAMPS
#define TLSAN_STAMPS 0   // 1: the diagnostic build with in-kernel cycle stamps (scripts/stamps.py)
#endif
// the correcting pass at the head of a training launch borrows the block (spec_fix_head, tlsan_attn.h): a 16-byte counter
// + FixLds; tlsan_attn.h, which sees tlsan_fix.h, asserts that this is 16 + FIX_LDS_BYTES
#define TLSAN_FIX_LDS_BYTES 14400
#define TLSAN_LDS_MAX_BYTES 163840   // what a workgroup may have on gfx950

template <typename G, bool TRAIN, bool LSTREAM, bool DROP, bool CSEG, typename At = ptrdiff_t>
struct AttnLds {
  // a region of T (float or int, both one dword): where it starts -- a T*, or a dword offset -- and its dwords
  template <typename T> using Ptr = std::conditional_t<std::is_pointer<At>::value, T*, At>;
  template <typename T> struct Rgn { Ptr<T> at = Ptr<T>(); int n = 0; };
  static constexpr int D = G::D, DH = G::DH, NB = G::NB, SPW = G::SPW, NW = G::NW, NSB = G::NSB, LSTR = G::LSTR;
  static constexpr bool SUPPORTED = NSB == 16 || (NSB == 8 && !LSTREAM);   // 8-sample workgroups: windows in registers only (k_fwd_bwd asserts it)
  static constexpr int LS = LSTREAM ? 1 : TLSAN_LS_MAX;             // positions held in registers
  static constexpr int LSC = LSTREAM ? TLSAN_LS_CAP : TLSAN_LS_MAX;  // position slots in the LDS tables
  static constexpr int WB = 2 * DH * DH + 2 * DH;    // floats of one attention block's weights
  static constexpr bool LKEY = NB == 1 && !LSTREAM;   // row keys reach a sample's lanes through the LDS (see g_item, P1, fetch_row_of)
  static constexpr int NLK = 16;                                    // session entries per chunk of keys
  // FLAT (streamed windows): the window positions of the workgroup's 16 samples form ONE list that is dealt out evenly
  // to its 16 column groups (a wavefront's lanes that share a sample slot) -- see P1.  Its entries, the per-sample
  // softmax statistics and the long-term vectors live in the LDS, where any group can reach them.
  static constexpr bool FLAT = LSTREAM && !DROP;   // (dropout keeps a window per column group: its pattern is indexed by (sample, position))
  static constexpr int NF = FLAT ? NSB * TLSAN_LS_CAP : 0;      // entries of the flat list (every window at the cap)
  // NB > 1 (d = 256): the LDS has no room for the per-sample statistics and long-term vectors beside the list -- they
  // go through global memory (FwdArgs.gStat, gLong: 32 KB per workgroup, L2-resident), the attention weights are
  // read from `dense` instead of an LDS copy, and the position tables keep session slots only
  static constexpr bool FLATG = FLAT && NB > 1;
  static constexpr bool STAT = FLAT && !FLATG && TRAIN;         // the per-sample statistics sMx / sIz live in the LDS
  static constexpr bool USE_SW = G::USE_SW && !FLATG;          // attention weights staged in LDS (when they fit)
  static constexpr int LSCP = FLAT ? 0 : LSC;                  // long slots of the position tables (FLAT: the list holds them)
  // PERM (two 16-channel blocks per column, d = 256): the weight fragments are re-read from the LDS at every position
  // (Geo::AT_USE), and read from the row-major copy that costs 8 two-dword reads with computed addresses per fragment,
  // four-way bank-conflicted (a fragment's lanes (q, r) read W[(16 kb + 4 q + s) * 32 + 16 jb + r]: the four q hit the
  // same banks) -- 26 M conflict cycles per launch, 28 % of the kernel's time (profiles/r04_pmc_d256_summary.txt).  The LDS
  // copy is therefore kept in FRAGMENT order, every matrix twice: table [pair][lane][4] with pair = the fragment's
  // (out block, in block) -- a fragment is NB * NB conflict-free 16-byte reads at constant offsets from the lane's base.
  // Per attention block: [W1 as T fragments | W2 as T | W1 as N | W2 as N | b1 | b2].
  static constexpr bool PERM = USE_SW && NB > 1 && !LSTREAM;   // (streamed windows with dropout keep the row-major copy: the 16 KB more do not fit beside their position tables)
  static constexpr int PP = NB * NB * 256;            // floats of one fragment table
  static constexpr int WBP = 4 * PP + 2 * DH;         // floats of one attention block's weights in fragment order
  static constexpr bool KEEP_A = G::KEEP_A && TRAIN && !LSTREAM;   // the long block's softmax weights stay in the LDS for the backward
  static constexpr int AW_WAVE = LS * NB * 256;       // floats of one wavefront's kept softmax weights
  // session slots of the position tables: the cap, or the batch's padded session length rounded up to 4 where that is what
  // fits -- CSEG keeps two such tables, FLATG has the list beside them, two 8-sample workgroups must fit a CU's LDS, and
  // the diagnostic stamps build needs its 2 KB of stamps beside the 160 KB the d = 128 training kernel fills
  static constexpr bool SNS_RT = CSEG || FLATG || NSB < 16 || TLSAN_STAMPS;

  // every region is a whole number of float4s whatever Sn is, so every region starts on one
  static_assert((NSB * LSTR) % 4 == 0 && NSB % 4 == 0 && (NSB * 2 * LSC) % 4 == 0 && (2 * WB) % 4 == 0 && (2 * WBP) % 4 == 0 &&
                NF % 4 == 0 && G::WSCR % 4 == 0 && AW_WAVE % 4 == 0, "regions of k_fwd_bwd's LDS block start on float4s");
  static_assert(2 * NF <= NSB * 2 * LSC, "FLAT: sFht and sFuh lie over sH");
  static_assert(!FLAT || !SUPPORTED || 32 * 3 * D <= NSB * LSTR + NW * G::WSCR, "partial states must fit sB + sT");
  static_assert(32 <= G::WSCR, "sPerm lies over the wavefront's scratch");

  // An aggregate: AttnLds{base, Sn, fuse_dk} runs the initializers below in order, each region starting where the one
  // before it ends -- in the kernel, inline, the chain of pointer + size steps it has always had.
  At base;        // the block: the kernel's float*, or 0
  int Sn;         // the batch's padded session length (FwdArgs.b.Sn)
  bool fuse_dk;   // this launch forms the dK partials itself (FwdArgs.fuse_dk)
  int SNS = SNS_RT ? ((Sn + 3) & ~3) : TLSAN_SN_CAP;   // session slots
  int PSTR = LSCP + SNS + 4;                            // per-sample position slots: long, session, 3 singles
  int P_TGT = LSCP + SNS, P_USR = P_TGT + 1, P_UC = P_TGT + 2;   // the singles' slots: target item, user, user's category
  // (sL exists in launches that fuse, and for FLAT's backward: at d = 64 it is what decides whether two workgroups fit a
  //  CU's LDS -- 8192 sequences, not fused: 77 us/step with it left out, 95 with it)
  bool has_sL = TRAIN && ((G::FUSE_DK && fuse_dk) || (FLAT && !FLATG));
  Rgn<float> A = {(Ptr<float>)base, NSB * LSTR};             // [NSB][LSTR]  long -> dbridge
  Rgn<float> B0 = {A.at + A.n, FLAT ? 0 : NSB * LSTR};        // [NSB][LSTR]  bridge -> dlong  (FLAT: placed in front of sT instead, see B; sL then starts where sB0 would)
  Rgn<float> L = {B0.at + B0.n, has_sL ? NSB * LSTR : 0};     // [NSB][LSTR]  long, kept for the fused dK product and for FLAT's backward
  Rgn<float> S = {L.at + L.n, NW * 4};                        // [NW][4] scalar staging
  Rgn<int> SK = {(Ptr<int>)(S.at + S.n), LKEY ? NW * 2 * SPW * NLK : 0};   // LKEY: [NW][2][SPW][NLK] item ids | categories of the current chunk of session entries
  Rgn<float> H = {(Ptr<float>)(SK.at + SK.n), NSB * 2 * LSC};   // [NSB][2*LS] hist_t and usert*hist_t of the pass  (FLAT: [2][NF], by flat index: Fht, Fuh)
  Rgn<float> W = {H.at + H.n, USE_SW ? (PERM ? 2 * WBP : 2 * WB) : 0};   // [2][WB] attention weights (W1,b1,W2,b2) of both blocks  (PERM: [2][WBP])
  Rgn<int> P = {(Ptr<int>)(W.at + W.n), TRAIN ? NSB * PSTR : 0};   // [NSB][PSTR] destination-sorted row of every use
  // CSEG (FwdArgs.cseg, many categories): the category half of an item use's gradient row goes to the category's own
  // segment of Gc -- its position, drawn from the category's cursor, sits in sPc beside the item position in sP
  Rgn<int> Pc = {P.at + P.n, (TRAIN && CSEG) ? NSB * PSTR : 0};
  Rgn<int> Fid = {Pc.at + Pc.n, NF};                          // FLAT: [NF] item id, category, (slot << 8 | position) of every list entry,
  Rgn<int> Fct = {Fid.at + Fid.n, NF};                        //       its destination rows (TRAIN), and below the per-sample statistics
  Rgn<int> Fst = {Fct.at + Fct.n, NF};
  Rgn<int> Fpos = {Fst.at + Fst.n, TRAIN ? NF : 0};
  Rgn<int> Fcpos = {Fpos.at + Fpos.n, (TRAIN && CSEG) ? NF : 0};
  Rgn<float> Mx = {(Ptr<float>)(Fcpos.at + Fcpos.n), STAT ? NSB * LSTR : 0};   // [NSB][LSTR] per-channel max of the window's scores
  Rgn<float> Iz = {Mx.at + Mx.n, STAT ? NSB * LSTR : 0};      // [NSB][LSTR] 1 / sum of exponentials
  Rgn<int> Bx = {(Ptr<int>)(Iz.at + Iz.n), FLATG ? NSB : 0};  // FLATG: [NSB] the slots' samples (rows of gStat / gLong)
  Rgn<int> Sb = {Bx.at + Bx.n, (!TRAIN && FLAT) ? NSB : 0};   // evaluation, FLAT: [NSB] the slots' samples (rows of FwdArgs.att0)
  Rgn<float> B = {FLAT ? (Ptr<float>)(Sb.at + Sb.n) : B0.at, NSB * LSTR};   // the bridge: FLAT here, in front of sT (see Part); otherwise it is sB0
  Rgn<float> T = {FLAT ? B.at + B.n : (Ptr<float>)Fid.at, NW * G::WSCR};    // per-wave transpose scratch / staging  (no flat list: nothing lies between sFid and here)
  Rgn<float> Aw = {T.at + T.n, KEEP_A ? NW * AW_WAVE : 0};    // [NW][LS][NB][64] the kept softmax weights, a float4 per lane
  Rgn<float> Stamp = {Aw.at + Aw.n, TLSAN_STAMPS ? NW * 32 * 2 : 0};   // [NW][32] 64-bit diagnostic stamps
  ptrdiff_t total = (Stamp.at + Stamp.n) - (Ptr<float>)base;  // dwords
  // overlays
  Rgn<float> Fht = {H.at, NF}, Fuh = {H.at + NF, NF};         // FLAT: hist_t and usert*hist_t by flat index, over sH
  // FLAT: the partial softmax states of P1, 32 slots of [3][D], lie over sB and sT (neither is touched before P2)
  Rgn<float> Part = {B.at, FLAT ? 32 * 3 * D : 0};
  Rgn<float> Perm = {T.at, 32};   // per wavefront, stride WSCR: the pass's slot assignment in the wave's own scratch (free until P3)

  // the bytes a launch asks for (a training launch: at least what spec_fix_head borrows)
  __host__ __device__ constexpr size_t bytes() const {
    const size_t b = sizeof(float) * (size_t)total;
    return (TRAIN && b < TLSAN_FIX_LDS_BYTES) ? (size_t)TLSAN_FIX_LDS_BYTES : b;
  }
  // what is known at compile time fits a workgroup's LDS: the whole block where the session slots are the cap, the part
  // that does not grow with Sn otherwise
  static constexpr bool fits() { return AttnLds<G, TRAIN, LSTREAM, DROP, CSEG>{0, 0, true}.bytes() <= TLSAN_LDS_MAX_BYTES; }
};

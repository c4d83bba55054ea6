// Prints the layout of k_fwd_bwd's dynamic LDS block (tlsan_attn_lds.h) over a grid of variants and run-time inputs; a
// host program that makes no HIP call (tests/test_attn_lds_cpu.py compiles it with --cuda-host-only and reads its output).
// Per case one line "<pair> train= lstream= drop= cseg= fuse= Sn= bytes=" in the format of tests/golden/fwd_lds_bytes.txt,
// then one line per region: "  <name> <offset> <size> <kind>", offsets and sizes in dwords, kind = r (a region of its
// own), v (the same, accessed as float4) or o (an overlay: lies over other regions on purpose).  A variant the kernel
// refuses to compile (AttnLds::SUPPORTED) has its total printed and "  unsupported" in place of the regions.
#include <cstdio>
#include "tlsan_attn_lds.h"

template <typename G, bool TRAIN, bool LSTREAM, bool DROP, bool CSEG>
static void dump_case(const char* name) {
  for (int fuse = 0; fuse < 2; ++fuse)
    for (int Sn : {0, 1, 3, 4, 5, 16, 44, 45, 48, 90, 96}) {
      const AttnLds<G, TRAIN, LSTREAM, DROP, CSEG> L = {0, Sn, fuse != 0};
      printf("%s train=%d lstream=%d drop=%d cseg=%d fuse=%d Sn=%d bytes=%zu\n", name, TRAIN, LSTREAM, DROP, CSEG, fuse, Sn, L.bytes());
      if (!L.SUPPORTED) { printf("  unsupported\n"); continue; }
#define R(name, kind) {"s" #name, L.name.at, L.name.n, kind}
      const struct { const char* name; ptrdiff_t at; int n; char kind; } rg[] = {
          R(A, 'v'), R(B0, 'v'), R(L, 'v'), R(S, 'v'), R(SK, 'r'), R(H, 'v'), R(W, 'v'), R(P, 'r'), R(Pc, 'r'), R(Fid, 'r'), R(Fct, 'r'), R(Fst, 'r'),
          R(Fpos, 'r'), R(Fcpos, 'r'), R(Mx, 'v'), R(Iz, 'v'), R(Bx, 'r'), R(Sb, 'r'),
          R(B, L.FLAT ? 'v' : 'o'),   // (without a flat list sB is sB0)
          R(T, 'v'), R(Aw, 'v'), R(Stamp, 'r'), R(Fht, 'o'), R(Fuh, 'o'), R(Part, 'o'), R(Perm, 'o')};
#undef R
      for (const auto& x : rg) printf("  %s %td %d %c\n", x.name, x.at, x.n, x.kind);
      printf("  total %td\n", L.total);
    }
}

template <int D, int DH, int NWV>
static void dump(const char* name) {
  using G = Geo<D, DH, NWV>;
  dump_case<G, false, false, false, false>(name);
  dump_case<G, false, true, false, false>(name);
  dump_case<G, true, false, false, false>(name);
  dump_case<G, true, false, false, true>(name);
  dump_case<G, true, false, true, false>(name);
  dump_case<G, true, false, true, true>(name);
  dump_case<G, true, true, false, false>(name);
  dump_case<G, true, true, false, true>(name);
  dump_case<G, true, true, true, false>(name);
  dump_case<G, true, true, true, true>(name);
}

int main() {
  dump<64, 8, 0>("d64h8"); dump<128, 16, 0>("d128h8"); dump<128, 16, 4>("d128h8w4"); dump<256, 32, 0>("d256h8");
  dump<64, 16, 0>("d64h4"); dump<128, 8, 0>("d128h16"); dump<128, 32, 0>("d128h4");
  return 0;
}

#!/usr/bin/env python3
"""Register / scratch report of every k_fwd_bwd instantiation: compiles the fused kernel's translation units for gfx950
with -Rpass-analysis=kernel-resource-usage (no GPU needed) and prints one line per variant.
  python scripts/kernel_registers.py [unit ...] > profiles/rNN_kernel_registers.txt
  python scripts/kernel_registers.py --all [unit ...]   every kernel of every unit of the build (or of the units named), one
                                              line each: the unit, the mangled name, VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes, occupancy"""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tlsan_amd", "csrc")
ALL = "--all" in sys.argv
UNITS = tuple(a for a in sys.argv[1:] if a != "--all") or ("tlsan_attn_d64", "tlsan_attn_d128", "tlsan_attn_d128w4", "tlsan_attn_d256", "tlsan_attn_d256s",
                               "tlsan_attn_d64h4", "tlsan_attn_d128h16", "tlsan_attn_d128h4")
sys.path.insert(0, ROOT)
from tlsan_amd.build import SOURCE_FLAGS, SOURCES   # (per-source compiler flags of the product build)
if ALL and len(sys.argv) == 2:
    UNITS = tuple(s[:-len(".hip")] for s in SOURCES)
def run(u):
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                            "-I" + CSRC] + SOURCE_FLAGS.get(u + ".hip", []) + ["--cuda-device-only", "-c", os.path.join(CSRC, u + ".hip"), "-o", os.path.join(td, "o.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        return r.stderr
with ThreadPoolExecutor(4) as ex:
    texts = list(ex.map(run, UNITS))
if ALL:
    rows = []
    for u, txt in zip(UNITS, texts):
        for m in re.findall(r"Function Name: (\S+).*?SGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S):
            n, sg, v, a, sc, occ, lds = m
            rows.append("%s %s vgpr=%s agpr=%s sgpr=%s scratch=%s lds=%s occ=%s" % (u, n, v, a, sg, sc, lds, occ))
    print("\n".join(sorted(rows)))
    sys.exit(0)
out = []
for txt in texts:
    for n, v, a, sc, occ, ss, vs in re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", txt, re.S):
        m = re.match(r"_Z9k_fwd_bwdILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELi(\d)ELb(\d)ELi(\d)ELb(\d)ELi(\d)E", n)
        if m:
            D, DH, tr, ls, dt, dr, mm, cs, nw = map(int, m.groups())
            out.append((D, DH, tr, ls, dt, dr, mm, cs, nw, int(v), int(a), int(sc), int(occ), int(ss), int(vs)))
out.sort()
print("# k_fwd_bwd<D, DH, TRAIN, LSTREAM, table bf16, DROP, matrix bf16, CSEG, NW> -- hipcc -Rpass-analysis=kernel-resource-usage, gfx950")
print("%4s %3s %5s %7s %4s %4s %4s %4s %3s | %5s %5s %12s %4s %10s %10s" % ("D", "DH", "TRAIN", "LSTREAM", "tbf", "DROP", "mbf", "CSEG", "NW", "VGPR", "AGPR", "scratch B/ln", "occ", "SGPR spill", "VGPR spill"))
for r in out:
    print("%4d %3d %5d %7d %4d %4d %4d %4d %3d | %5d %5d %12d %4d %10d %10d" % r)

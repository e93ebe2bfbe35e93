"""Static instruction counts per marked section of the bit-plane coder at depth D (hipcc -S -DBP_MARKS): which part of the
window loop the vector instructions sit in.  usage: python tools/isa_sections.py [depth] [planes] [lazy]   (needs hipcc)
planes 1: k_lz4_bitplanes_uni<D> (bit-plane input; its plain and exception-aware paths both count), 0: k_lz4_bitplanes<D>
(int8 input).  lazy 1: the instantiation with the lazy rule (built for depths 2 and 12), 0 (default): without.
Counts are per textual section between markers, in listing order (a basic block the compiler moved elsewhere is
attributed to where it landed), so read them as a map, not as a cycle count."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
depth = int(sys.argv[1]) if len(sys.argv) > 1 else 2
planes = int(sys.argv[2]) if len(sys.argv) > 2 else 1   # 1: the plane-input kernel, 0: int8 input
lazy = int(sys.argv[3]) if len(sys.argv) > 3 else 0
kernel = f"_Z19k_lz4_bitplanes_uniILi{depth}ELb{lazy}E" if planes else f"_Z15k_lz4_bitplanesILi{depth}ELb{lazy}E"
out = "/tmp/lz4bits_marks.s"
subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", "-DBP_MARKS",
                       "-I", os.path.join(ROOT, "include"), "-o", out,
                       os.path.join(ROOT, "haplohyped_varawareml_amd", "csrc", "lz4bits.hip")], stderr=subprocess.DEVNULL)
inside, sec = False, "entry"
cnt = collections.OrderedDict()
for line in open(out):
    if line.startswith(kernel):
        inside = True
        continue
    if not inside:
        continue
    t = line.strip()
    if t.startswith("s_endpgm") and sec == "loop_done":
        pass
    if t.startswith(".section") or t.startswith(".rodata"):
        break
    m = re.match(r"; ==MARK (\w+)", t)
    if m:
        sec = m.group(1)
        continue
    if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
        continue
    op = t.split()[0]
    kind = "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "lds" if op.startswith("ds_") else \
        "vmem" if op.startswith(("global_", "flat_", "buffer_", "scratch_")) else "other"
    cnt.setdefault(sec, collections.Counter())[kind] += 1
    if op == "s_waitcnt" and "lgkmcnt" in t:
        cnt[sec]["lgkm_wait"] += 1          # a wait on LDS / scalar-memory results: one link of the wave's dependent chain
print(f"{'k_lz4_bitplanes_uni' if planes else 'k_lz4_bitplanes'}<{depth}{', lazy' if lazy else ''}>: instructions in the listing after each marker")
for k, c in cnt.items():
    print(f"  {k:12s} valu {c['valu']:5d}  salu {c['salu']:5d}  lds {c['lds']:4d}  vmem {c['vmem']:4d}  waits on lds {c['lgkm_wait']:3d}")

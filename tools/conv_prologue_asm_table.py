#!/usr/bin/env python3
"""Static (no GPU): where the first loads of every k_conv3x3_mfma instantiation sit in its instruction stream.
Compiles phiseg_code_amd/csrc/conv_mfma.hip to gfx950 assembly (hipcc -O3 --cuda-device-only -S, extra flags passed through, e.g.
-DPHX_CONV_LOADS_FIRST=0) and prints, per instantiation <BN,NA,FAST16,BIASACT,NW,SPLITK,DUAL,FGN>: instructions in the kernel, index of
the first buffer_load, of the last of the first chunk's NA + NB loads, of the first MFMA, the largest run of instructions between two
consecutive loads of the first chunk, and whether the filter-slab loads (NB of them, told by their descriptor registers) come first.
usage: conv_prologue_asm_table.py [--src FILE] [--asm FILE.s (kept)] [hipcc flags ...]"""
import os
import re
import subprocess
import sys
import tempfile

here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
src = os.path.join(here, "phiseg_code_amd", "csrc", "conv_mfma.hip")
keep = None
while args[:1] in (["--src"], ["--asm"]):
    if args[0] == "--src":
        src = args[1]
    else:
        keep = args[1]
    args = args[2:]
with tempfile.TemporaryDirectory() as tmp:
    out = keep or os.path.join(tmp, "conv_mfma.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
                           "-I", os.path.join(here, "phiseg_code_amd", "csrc")] + args + [src, "-o", out])
    lines = open(out).read().split("\n")

rows, name, body = [], None, []
for ln in lines:
    m = re.match(r"^(_Z\w*k_conv3x3_mfma\w*):", ln)
    if m:
        name, body = m.group(1), []
        continue
    if name is None:
        continue
    t = ln.strip()
    if not t or t.startswith((".", ";")) or t.endswith(":"):
        continue
    body.append(t)
    if t.startswith("s_endpgm"):
        rows.append((name, body))
        name = None
print("%-34s %6s %6s %6s %6s %7s %s" % ("<BN,NA,FAST16,BIASACT,NW,SPLITK,DUAL,FGN>", "instr", "load0", "loadN", "mfma0", "max gap", "slab loads first"))
for mangled, body in sorted(rows):
    ta = [int(v) for v in re.findall(r"L[ib](\d+)E", mangled[:mangled.index("EEv")] + "E")]      # template arguments of the mangled name
    na, nb = ta[1], (9 * ta[0] * 4 + ta[4] * 64 - 1) // (ta[4] * 64)
    mf = next(i for i, t in enumerate(body) if t.startswith("v_mfma"))
    ld = [i for i, t in enumerate(body[:mf]) if t.startswith("buffer_load")][:na + nb]      # the first chunk's loads (later ones: the prefetch of the next)
    gaps = [b - a - 1 for a, b in zip(ld, ld[1:])]
    rsrc = [re.search(r"s\[\d+:\d+\]", body[i]).group(0) for i in ld]                          # descriptor registers: filter vs. input
    slab_first = len(set(rsrc[:nb])) == 1 and rsrc[nb] != rsrc[0]
    print("%-34s %6d %6d %6d %6d %7d %s" % ("<" + ",".join(str(v) for v in ta) + ">", len(body), ld[0], ld[-1], mf, max(gaps), "yes" if slab_first else "no"))

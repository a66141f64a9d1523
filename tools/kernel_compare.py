#!/usr/bin/env python3
"""usage: tools/kernel_compare.py <parent tree> <change tree>
Per translation unit of both libraries (the objects build() leaves in csrc/_build/<lib>/): the gfx950 code object is taken out of
the offload bundle, disassembled and split per kernel; metadata (llvm-readelf --notes) and ISA are compared kernel by kernel.
A kernel that only moved (another kernel of its unit changed its size) is counted apart from one whose code or metadata differs."""
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
def code_object(obj):
    data = open(obj, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    if i < 0:
        return None                      # a unit without device code
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, s, l = struct.unpack_from("<QQQ", data, off)
        off += 24
        name = data[off:off + l]
        off += l
        if b"gfx950" in name:
            return data[i + o:i + o + s]
    raise SystemExit("no gfx950 code object in " + obj)
def kernels(obj):
    co = code_object(obj)
    if co is None:
        return None, {}, {}
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        return (co,) + read_kernels(f.name)


def read_kernels(tmp):
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", tmp], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
        blk = blk.split("\namdhsa.target")[0]
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = blk
    dis = subprocess.run([LLVM + "/llvm-objdump", "-d", tmp], capture_output=True, text=True, check=True).stdout
    isa = {}
    for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^\n?[0-9a-f]+ <|\Z)", dis, re.S | re.M):
        isa[m.group(1)] = m.group(2)
    return meta, isa
def unplaced(text):
    """a kernel's disassembly, instruction words included, without the addresses (every instruction's, and the branch targets
    llvm-objdump resolves)"""
    return re.sub(r"// [0-9A-F]+:", "//", re.sub(r" <[^>]+>$", "", text, flags=re.M))
parent, change = sys.argv[1:3]
tot = [0, 0, 0, 0]
for lib in ("libmcl_hip_engine.so", "libmcl_hip_engine_legacy.so"):
    for o in sorted(glob.glob(f"{change}/monte_carlo_localization_amd/csrc/_build/{lib}/*.o")):
        tu = os.path.basename(o)
        cc, mc, ic = kernels(o)
        po = f"{parent}/monte_carlo_localization_amd/csrc/_build/{lib}/{tu}"
        if not os.path.exists(po):           # a unit the parent does not have
            print(f"{lib:30s} {tu:18s} new unit: kernels {len(mc)}")
            tot[1] += len(mc)
            continue
        cp, mp, ip = kernels(po)
        differ = [k for k in sorted(set(mp) | set(mc)) if mp.get(k) != mc.get(k) or ip.get(k) != ic.get(k) or k not in ip]
        # a kernel behind one that changed its size: the same metadata and instruction words at another address
        moved = [k for k in differ if mp.get(k) == mc.get(k) and k in ip and k in ic and unplaced(ip[k]) == unplaced(ic[k])]
        print(f"{lib:30s} {tu:18s} kernels parent {len(mp):3d} change {len(mc):3d}  differing {len(differ) - len(moved)}  moved only {len(moved)}"
              f"  code object bytes {'equal' if cp == cc else 'differ'}")
        for k in differ:
            if k not in moved:
                print("    DIFFERS:", k)
        tot = [tot[0] + len(mp), tot[1] + len(mc), tot[2] + len(differ) - len(moved), tot[3] + len(moved)]
print(f"total: parent {tot[0]} kernels, change {tot[1]}, differing {tot[2]}, moved only {tot[3]}")

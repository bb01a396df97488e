#!/usr/bin/env python3
"""The resource table of profiles/relax_kernel_resources.txt and profiles/resolve_kernel_resources.txt from the compiler's
remarks and the disassembly.  Works on any kernel source file:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only --no-gpu-bundle-output \\
        -Rpass-analysis=kernel-resource-usage -c -o A.co rustronomy-watershed_amd/csrc/ws_relax.hip 2> A.remarks
  relax_kernel_resources.py [--no-padding] PARENT.remarks PARENT.co THIS.remarks THIS.co

Kernels that moved between files: give a side several files, comma separated (A.remarks,B.remarks A.co,B.co), and
--no-padding (below): profiles/resolve_kernel_resources.txt was made that way, profiles/relax_kernel_resources.txt without.

Columns: VGPRs, SGPRs (total), scratch bytes per lane, occupancy in waves per SIMD, SGPRs spilled, VGPRs spilled, LDS bytes
per workgroup, instructions (disassembled lines between a kernel's symbol and the next; --no-padding leaves out the s_nop /
s_code_end lines after a kernel's last instruction, which depend on what follows the kernel in its file)."""
import os
import re
import shutil
import subprocess
import sys

KEYS = ["VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def objdump():
    """llvm-objdump from PATH, else from the ROCm tree (ROCM_PATH, default /opt/rocm)."""
    return shutil.which("llvm-objdump") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    return re.sub(r"\(.*", "", name.replace("void ", "").replace("wsk::", ""))


def table(remarks, code_object, no_padding=False):
    if "," in remarks:      # several files on this side
        merged = {}
        for r, c in zip(remarks.split(","), code_object.split(",")):
            merged.update(table(r, c, no_padding))
        return merged
    rows, name = {}, None
    for line in open(remarks):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            rows[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
        if m and name:
            rows[name][m.group(1)] = int(m.group(2))
    dis = subprocess.run([objdump(), "-d", code_object], capture_output=True, text=True).stdout
    cur, pad = None, 0
    for line in dis.split("\n"):
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur, pad = m.group(1), 0
            continue
        if cur in rows and re.match(r"\s+\S+.*//", line):
            if no_padding and re.match(r"\s+(s_nop|s_code_end)\b", line):
                pad += 1      # counted only if an instruction follows
            else:
                rows[cur]["instrs"] = rows[cur].get("instrs", 0) + 1 + pad
                pad = 0
    names = demangle(list(rows))
    return {short(names[k]): [v.get(c, -1) for c in KEYS] + [v.get("instrs", -1)] for k, v in rows.items()}


def main():
    args = [x for x in sys.argv[1:] if x != "--no-padding"]
    no_padding = len(args) != len(sys.argv) - 1
    a, b = table(args[0], args[1], no_padding), table(args[2], args[3], no_padding)
    fmt = "%6d %5d %7d %3d %6d %6d %7d %6d"
    print("%-52s | %-52s | %s" % ("kernel", "parent:  VGPR  SGPR scratch occ Sspill Vspill     LDS instrs", "this commit"))
    differs = []
    for k in sorted(set(a) | set(b)):
        ra, rb = a.get(k), b.get(k)
        print("%-52s | %-52s | %s" % (k, fmt % tuple(ra) if ra else "-", "=" if ra == rb else (fmt % tuple(rb) if rb else "-")))
        if ra != rb:
            differs.append(k)
    print("\ndiffering rows: %s" % (", ".join(differs) if differs else "none"))


if __name__ == "__main__":
    main()

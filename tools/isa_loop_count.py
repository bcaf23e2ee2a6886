#!/usr/bin/env python3
"""Instruction census of a kernel's main loop in a hipcc assembly listing (-S --offload-device-only).

  python tools/isa_loop_count.py conv_kernels.s 'k_conv3x3_win_s3ILi4ELi32ENS_13EpiStoreStatsELb1'

Takes the first kernel whose mangled name contains the pattern, finds its depth-1 loop (the blocks LLVM
marks "in Loop: Header=..." plus the header itself) and prints how many VALU, MFMA, LDS, VMEM, SALU and
wait instructions one trip of that loop holds (every block counted once: the upper bound of a stage
that takes all its branches), with the kernel's VGPR count and occupancy.
"""
import re
import sys


def main():
    path, pat = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and pat in l and l.rstrip().split(":")[0].endswith("E"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.end_amdhsa_kernel") or ".Lfunc_end" in lines[i])
    body = lines[start:end]
    in_loop, counts = False, {}
    for l in body:
        if re.match(r"^(\.LBB|; %bb)", l):
            in_loop = "Loop Header" in l or "in Loop:" in l
            continue
        if not in_loop:
            continue
        m = re.match(r"^\t([a-z_0-9]+)", l)
        if not m:
            continue
        op = m.group(1)
        if op.startswith("v_mfma"):
            k = "mfma"
        elif op.startswith("v_"):
            k = "valu"
        elif op.startswith("ds_read"):
            k = "ds_read"
        elif op.startswith("ds_write"):
            k = "ds_write"
        elif op.startswith("buffer_load") and l.rstrip().endswith("lds"):
            k = "lds_dma"
        elif op.startswith(("buffer_", "global_", "flat_")):
            k = "vmem"
        elif op in ("s_waitcnt", "s_barrier", "s_nop"):
            k = op
        elif op.startswith("s_"):
            k = "salu"
        else:
            k = "other"
        counts[k] = counts.get(k, 0) + 1
    tail = "\n".join(lines[end:end + 80])
    regs = re.search(r"; NumVgprs: (\d+)", tail)
    occ = re.search(r"; Occupancy: (\d+)", tail)
    print(lines[start].split(":")[0])
    print("  loop:", ", ".join(f"{k} {v}" for k, v in sorted(counts.items())))
    print("  vgprs", regs.group(1) if regs else "?", "occupancy", occ.group(1) if occ else "?")


if __name__ == "__main__":
    main()

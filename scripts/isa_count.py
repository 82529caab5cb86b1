#!/usr/bin/env python3
"""Static instruction counts of one kernel in a hipcc --save-temps assembly file (*.s), whole and per barrier-delimited region.

    python scripts/isa_count.py FILE.s MANGLED_SUBSTRING

Prints the kernel's VGPR / scratch figures from its .amdhsa block, the number of vector (v_*), scalar (s_*), LDS (ds_*) and memory instructions, the
counts of a few opcodes the match step is made of, and the same per region between two s_barrier instructions in program order.  A tile body of k_lzm
is the run of regions between the barrier that ends one tile and the next such barrier: the FULL instance and the general one follow each other in the
file, each with its own two barriers (one before the window chunk, one at the tile's end).  The compiler lays blocks out in its own order: which
region is the FULL body shows in the code (the general one compares every position with the tile's and the segment's end and clamps at the
block's), and the first of the two regions also holds the tile loop's head.  LAB_LOG.md 6.3 names the regions it quotes.
"""
import collections
import re
import sys


def kernel_text(path, sub):
    lines = open(path).read().split("\n")
    start = end = None
    for i, ln in enumerate(lines):
        if start is None and re.match(r"^_Z\S*:", ln) and sub in ln:
            start = i
        elif start is not None and ln.startswith("\t.end_amdhsa_kernel"):
            end = i
            break
    if start is None or end is None:
        sys.exit("kernel not found: " + sub)
    return lines[start:end]


def classify(op):
    if op.startswith("v_"):
        return "vector"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "memory"
    return None


def main():
    path, sub = sys.argv[1], sys.argv[2]
    text = kernel_text(path, sub)
    print(text[0].rstrip(":"))
    for ln in text:
        m = re.search(r"\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size)\s+(\S+)", ln)
        if m:
            print("  %s = %s" % m.groups())
    watch = ("v_alignbyte_b32", "v_alignbit_b32", "v_ffbl_b32", "v_min3_u32", "v_xor_b32_e32", "v_lshrrev_b32_e32", "ds_read")
    total = collections.Counter()
    regions = [collections.Counter()]
    for ln in text:
        m = re.match(r"^\t([a-z][a-z0-9_]+)\b", ln)
        if not m:
            continue
        op = m.group(1)
        kind = classify(op)
        if kind is None:
            continue
        for c in (total, regions[-1]):
            c[kind] += 1
            for w in watch:
                if op.startswith(w):
                    c[w] += 1
        if op == "s_barrier":
            regions.append(collections.Counter())
    fmt = lambda c: "  ".join("%s %d" % (k, c[k]) for k in ("vector", "scalar", "lds", "memory") + watch)
    print("whole kernel:", fmt(total))
    for i, r in enumerate(regions):
        print("region %2d: %s" % (i, fmt(r)))


if __name__ == "__main__":
    main()

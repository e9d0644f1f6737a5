#!/usr/bin/env python3
"""Static instruction census of one kernel per source region: VALU / SALU / SMEM / LDS / VMEM counts from the
line-table assembly (tools/valu_lines.py counts per line of one file; this one per region of any file).

Build the line-table assembly first:
  hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -gline-tables-only --cuda-device-only \
        -S -o rust-ray-tracing_amd/build/dbg.s rust-ray-tracing_amd/csrc/rt_kernel.hip

Usage: isa_census.py [--asm PATH] [--top N] KERNEL [NAME=]FILE:FIRST-LAST ...
  KERNEL  a substring of the mangled name (the first kernel that has it)
  region  the instructions whose source line is FIRST..LAST of the file whose path ends in FILE; an instruction
          belongs to the first region listed that holds its line, so list a nested region before its parent
Every other line of a listed file is summed as "FILE, other lines", every other file as "other files", and the
instructions the compiler gave line 0 (or none) as "no source line".  --top N (default 3) names each region's N
most frequent VALU opcodes.  The counts are static: an instruction in a loop counts once.
"""
import argparse
import collections
import re


def unit(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vmem"
    return "other"


def census(asm, kernel):
    """-> (mangled name, {(file, line) or None: Counter of opcodes})"""
    t = open(asm).read()
    files = {m.group(1): m.group(3) for m in re.finditer(r'\.file\s+(\d+)\s+"([^"]*)"\s+"([^"]+)"', t)}
    files.update({m.group(1): m.group(2) for m in re.finditer(r'\.file\s+(\d+)\s+"([^"]+)"\s*(?:md5|$)', t, re.M)
                  if m.group(1) not in files})
    name = next(m.group(1) for m in re.finditer(r"^(\S+):", t, re.M) if kernel in m.group(1))
    start = t.index(name + ":")
    body = t[start:t.index(".Lfunc_end", start)].split("\n")[1:]
    ops = collections.defaultdict(collections.Counter)
    cur = None
    for line in body:
        s = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (files.get(m.group(1), "?"), int(m.group(2))) if int(m.group(2)) else None
            continue
        if not s or s.startswith((";", ".")) or s.split(";")[0].strip().endswith(":"):
            continue
        ops[cur][s.split()[0]] += 1
    return name, ops


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", default="rust-ray-tracing_amd/build/dbg.s")
    ap.add_argument("--top", type=int, default=3)
    ap.add_argument("kernel")
    ap.add_argument("regions", nargs="*")
    a = ap.parse_args()
    regions = []
    for r in a.regions:
        label, _, spec = r.rpartition("=")
        f, _, span = spec.rpartition(":")
        lo, _, hi = span.partition("-")
        regions.append((label or spec, f, int(lo), int(hi or lo)))
    name, ops = census(a.asm, a.kernel)
    rows = collections.OrderedDict((r[0], collections.Counter()) for r in regions)
    for _, f, _, _ in regions:
        rows.setdefault(f + ", other lines", collections.Counter())
    rows["other files"] = collections.Counter()
    rows["no source line"] = collections.Counter()
    for key, c in ops.items():
        if key is None:
            rows["no source line"].update(c)
            continue
        f, ln = key
        hit = next((r[0] for r in regions if f.endswith(r[1]) and r[2] <= ln <= r[3]), None)
        if hit is None:
            hit = next((r[1] + ", other lines" for r in regions if f.endswith(r[1])), "other files")
        rows[hit].update(c)
    print(name)
    print(f"{'region':44s} {'VALU':>6s} {'SALU':>6s} {'SMEM':>5s} {'LDS':>5s} {'VMEM':>5s}  most frequent VALU")
    total = collections.Counter()
    for label, c in rows.items():
        u = collections.Counter()
        for op, n in c.items():
            u[unit(op)] += n
        total.update(u)
        top = collections.Counter({op: n for op, n in c.items() if unit(op) == "valu"}).most_common(a.top)
        print(f"{label:44s} {u['valu']:6d} {u['salu']:6d} {u['smem']:5d} {u['lds']:5d} {u['vmem']:5d}  "
              + ", ".join(f"{n} {op}" for op, n in top))
    print(f"{'total':44s} {total['valu']:6d} {total['salu']:6d} {total['smem']:5d} {total['lds']:5d} {total['vmem']:5d}")


if __name__ == "__main__":
    main()

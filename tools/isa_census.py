#!/usr/bin/env python3
"""Static instruction census of one kernel per source region: VALU / SALU / SMEM / LDS / VMEM counts from the
line-table assembly (tools/valu_lines.py counts per line of one file; this one per region of any file).

Build the line-table assembly first:
  hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17 -gline-tables-only --cuda-device-only \
        -S -o rust-ray-tracing_amd/build/dbg.s rust-ray-tracing_amd/csrc/rt_kernel.hip

Usage: isa_census.py [--asm PATH] [--top N] [--weights PATH] KERNEL [NAME=]FILE:FIRST-LAST ...
  KERNEL  a substring of the mangled name (the first kernel that has it)
  region  the instructions whose source line is FIRST..LAST of the file whose path ends in FILE; an instruction
          belongs to the first region listed that holds its line, so list a nested region before its parent
Every other line of a listed file is summed as "FILE, other lines", every other file as "other files", and the
instructions the compiler gave line 0 (or none) as "no source line".  --top N (default 3) names each region's N
most frequent VALU opcodes.  The counts are static: an instruction in a loop counts once.

The "cyc" column weights each VALU instruction by the issue cost of its form, in SIMD-cycles per wave-instruction:
co-issuing (an add, sub, mul, fma, mov or and with every source in a VGPR), the same with an SGPR or constant
source, single-issue, transcendental.  The classes, their opcodes and their costs are data, tools/issue_weights.json
(from profiles/r06/issue_counters.txt); "co/op/1x/tr" counts the region's VALU instructions per class.  The costs
were measured one form at a time, so the column ranks regions; it does not predict a kernel's time.
"""
import argparse
import collections
import json
import os
import re

WEIGHTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "issue_weights.json")
CLASSES = ("coissue", "operand", "single", "trans")   # printed; trans64 counts with trans


def issue_class(op, operands, w):
    """The issue class (a key of w["cycles"]) of one VALU instruction: opcode without its encoding suffix, and the
    source operands as written (everything after the destination)."""
    base = re.sub(r"_(e32|e64)$", "", op)
    if base in w["trans_ops"]:
        return "trans"
    if base in w["trans64_ops"]:
        return "trans64"
    if base not in w["coissue_ops"]:
        return "single"          # also every _dpp / _sdwa form: the suffix is not stripped
    srcs = [re.sub(r"^(-|\||neg\(|abs\()+|[|)]+$", "", t.strip()) for t in operands.split(",")[1:]]
    srcs = [t for t in srcs if t and not re.match(r"^(op_sel|op_sel_hi|neg_lo|neg_hi|clamp|mul:|div:)", t)]
    return "coissue" if srcs and all(re.match(r"^v(\d+|\[\d+:\d+\])$", t) for t in srcs) else "operand"


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


def census(asm, kernel, weights=None):
    """-> (mangled name, {(file, line) or None: Counter of opcodes}, {the same keys: Counter of issue classes})"""
    t = open(asm).read()
    files = {m.group(1): m.group(3) for m in re.finditer(r'\.file\s+(\d+)\s+"([^"]*)"\s+"([^"]+)"', t)}
    files.update({m.group(1): m.group(2) for m in re.finditer(r'\.file\s+(\d+)\s+"([^"]+)"\s*(?:md5|$)', t, re.M)
                  if m.group(1) not in files})
    name = next(m.group(1) for m in re.finditer(r"^(\S+):", t, re.M) if kernel in m.group(1))
    start = t.index(name + ":")
    body = t[start:t.index(".Lfunc_end", start)].split("\n")[1:]
    ops = collections.defaultdict(collections.Counter)
    cls = collections.defaultdict(collections.Counter)
    cur = None
    for line in body:
        s = line.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            cur = (files.get(m.group(1), "?"), int(m.group(2))) if int(m.group(2)) else None
            continue
        if not s or s.startswith((";", ".")) or s.split(";")[0].strip().endswith(":"):
            continue
        op = s.split()[0]
        ops[cur][op] += 1
        if weights and unit(op) == "valu":
            cls[cur][issue_class(op, s.split(";")[0][len(op):], weights)] += 1
    return name, ops, cls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", default="rust-ray-tracing_amd/build/dbg.s")
    ap.add_argument("--top", type=int, default=3)
    ap.add_argument("--weights", default=WEIGHTS)
    ap.add_argument("kernel")
    ap.add_argument("regions", nargs="*")
    a = ap.parse_args()
    regions = []
    for r in a.regions:
        label, _, spec = r.rpartition("=")
        f, _, span = spec.rpartition(":")
        lo, _, hi = span.partition("-")
        regions.append((label or spec, f, int(lo), int(hi or lo)))
    with open(a.weights) as f:
        w = json.load(f)
    name, ops, cls = census(a.asm, a.kernel, w)
    rows = collections.OrderedDict((r[0], collections.Counter()) for r in regions)
    rcls = collections.defaultdict(collections.Counter)
    for _, f, _, _ in regions:
        rows.setdefault(f + ", other lines", collections.Counter())
    rows["other files"] = collections.Counter()
    rows["no source line"] = collections.Counter()
    for key, c in ops.items():
        if key is None:
            rows["no source line"].update(c)
            rcls["no source line"].update(cls[key])
            continue
        f, ln = key
        hit = next((r[0] for r in regions if f.endswith(r[1]) and r[2] <= ln <= r[3]), None)
        if hit is None:
            hit = next((r[1] + ", other lines" for r in regions if f.endswith(r[1])), "other files")
        rows[hit].update(c)
        rcls[hit].update(cls[key])

    def cyc(k):
        return sum(n * w["cycles"][c] for c, n in k.items())

    def forms(k):
        return "/".join(str(k[c] + (k["trans64"] if c == "trans" else 0)) for c in CLASSES)
    print(name)
    print(f"{'region':44s} {'VALU':>6s} {'cyc':>8s} {'co/op/1x/tr':>18s} {'SALU':>6s} {'SMEM':>5s} {'LDS':>5s} {'VMEM':>5s}  "
          "most frequent VALU")
    total, tcls = collections.Counter(), collections.Counter()
    for label, c in rows.items():
        u = collections.Counter()
        for op, n in c.items():
            u[unit(op)] += n
        total.update(u)
        tcls.update(rcls[label])
        top = collections.Counter({op: n for op, n in c.items() if unit(op) == "valu"}).most_common(a.top)
        print(f"{label:44s} {u['valu']:6d} {cyc(rcls[label]):8.0f} {forms(rcls[label]):>18s} {u['salu']:6d} {u['smem']:5d} "
              f"{u['lds']:5d} {u['vmem']:5d}  " + ", ".join(f"{n} {op}" for op, n in top))
    print(f"{'total':44s} {total['valu']:6d} {cyc(tcls):8.0f} {forms(tcls):>18s} {total['salu']:6d} {total['smem']:5d} "
          f"{total['lds']:5d} {total['vmem']:5d}")


if __name__ == "__main__":
    main()

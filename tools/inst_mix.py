#!/usr/bin/env python3
"""The instruction mix of one kernel of a gfx950 listing (hipcc
--cuda-device-only -S with the unit's flags from the Makefile), whole, per
loop and, when the listing carries line tables (-gline-tables-only), per
source region.

Classes, by mnemonic prefix only: VALU (v_), lane moves (v_readlane /
v_writelane / v_readfirstlane: SGPR spill traffic and broadcasts), SALU (s_),
branches (s_branch, s_cbranch_), waits (s_waitcnt, s_nop, s_sleep), scalar
memory (s_load_, s_buffer_load_), LDS (ds_), vector memory (global_, buffer_,
flat_, scratch_).  A loop is the range of a backward branch; nested loops are
listed innermost last, each with its own totals.  --weights FILE: a JSON object
{"<first line>-<last line>": calls, ...} multiplies a source region's static
counts by how often it runs (the lane statistics' call counts), so that
regions can be ordered by what they issue.

usage: tools/inst_mix.py <listing.s> <kernel substring> [--top N] [--salu]
                         [--regions FILE:FIRST-LAST ...] [--weights FILE]
"""
import argparse
import collections
import json
import re

CLASSES = ("VALU", "lane", "SALU", "branch", "wait", "smem", "LDS", "vmem")


def classify(m):
    if m.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith(("s_branch", "s_cbranch_")):
        return "branch"
    if m.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if m.startswith(("s_load_", "s_buffer_load_")):
        return "smem"
    if m.startswith("s_"):
        return "SALU"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return None


def kernel_body(path, pat):
    """[(mnemonic, operands, file id, line)], labels {name: index}, files {id: name} of the first kernel matching pat."""
    ins, labels, files = [], {}, {}
    inside, loc = False, (0, 0)
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        m = re.match(r"\s*\.file\s+(\d+)\s+(?:\"([^\"]*)\"\s+)?\"([^\"]*)\"", line)
        if m:
            files[int(m.group(1))] = m.group(3)
        m = re.match(r"^(\S+):\s*$", line)
        if m and not line.startswith("\t"):
            name = m.group(1)
            if not inside and not name.startswith(".") and pat in name:
                inside = True
                continue
            if inside:
                labels[name] = len(ins)
            continue
        if not inside:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".end_amdhsa_kernel"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        if not s or s.startswith("."):
            continue
        parts = s.split(None, 1)
        if classify(parts[0]) is not None:
            ins.append((parts[0], parts[1] if len(parts) > 1 else "", loc[0], loc[1]))
    return ins, labels, files


def mix(rows):
    c = collections.Counter(classify(r[0]) for r in rows)
    return c


def fmt(c):
    return " ".join(f"{k} {c.get(k, 0):>5}" for k in CLASSES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--top", type=int, default=12, help="loops to print, largest scalar side first")
    ap.add_argument("--salu", action="store_true", help="the SALU mnemonics of the kernel by count")
    ap.add_argument("--regions", nargs="*", default=[], help="FILE:FIRST-LAST source regions (needs line tables)")
    ap.add_argument("--weights", default=None)
    a = ap.parse_args()
    ins, labels, files = kernel_body(a.listing, a.kernel)
    if not ins:
        raise SystemExit(f"no kernel matching {a.kernel}")
    total = mix(ins)
    print(f"kernel: {len(ins)} instructions\n  {fmt(total)}")
    if a.salu:
        by = collections.Counter(r[0] for r in ins if classify(r[0]) == "SALU")
        for k, v in by.most_common(12):
            print(f"  {k:28s} {v}")
    # loops: a branch whose target label stands at or before it
    loops = []
    for i, (m, ops, _, _) in enumerate(ins):
        if classify(m) != "branch":
            continue
        t = ops.split(",")[-1].strip()
        if t in labels and labels[t] <= i:
            loops.append((labels[t], i))
    loops = sorted(set(loops))
    print(f"{len(loops)} loops (backward branches)")
    rows = []
    for lo, hi in loops:
        c = mix(ins[lo:hi + 1])
        depth = sum(1 for l2, h2 in loops if l2 <= lo and hi <= h2) - 1
        side = c["SALU"] + c["branch"] + c["wait"] + c["smem"]
        rows.append((side, lo, hi, depth, c))
    for side, lo, hi, depth, c in sorted(rows, reverse=True)[:a.top]:
        print(f"  [{lo:>5}..{hi:>5}] depth {depth} {hi - lo + 1:>5} instr, scalar side {side:>4}: {fmt(c)}")
    if a.regions:
        weights = json.load(open(a.weights)) if a.weights else {}
        if not any(r[3] for r in ins):
            raise SystemExit("the listing has no line tables: compile it with -gline-tables-only")
        out = []
        for spec in a.regions:
            f, span = spec.rsplit(":", 1)
            first, last = (int(x) for x in span.split("-"))
            ids = {k for k, v in files.items() if v.endswith(f)}
            c = mix([r for r in ins if r[2] in ids and first <= r[3] <= last])
            w = float(weights.get(spec, 1.0))
            out.append((w * (c["SALU"] + c["branch"] + c["wait"] + c["smem"]), spec, w, c))
        for dyn, spec, w, c in sorted(out, reverse=True):
            print(f"  {spec:40s} x {w:g}: scalar side {dyn:g}; static {fmt(c)}")


if __name__ == "__main__":
    main()

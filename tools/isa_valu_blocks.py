#!/usr/bin/env python3
"""VALU instructions per basic block of one kernel in a hipcc --save-temps .s file.

  tools/isa_valu_blocks.py kernels_match-hip-amdgcn-amd-amdhsa-gfx950.s match_kernelILb1E

One line per block: label, first line, VALU count, and the counts of the instructions that tell the
regions of match_kernel apart (SADs, LDS-DMA, DPP, readlane, bpermute, permlane swaps, global loads /
stores, branches back = loops).  The per-region table of profiles/EXPERIMENTS.md is read off this.
"""
import re
import sys

MARKS = [("sad", r"v_sad_"), ("dma", r"global_load_lds"), ("dpp", r"_dpp|row_ror|row_shr"), ("rdl", r"v_readlane|v_readfirstlane"),
         ("bperm", r"ds_bpermute"), ("swap", r"v_permlane"), ("gld", r"global_load_(?!lds)"), ("sld", r"s_load_|s_buffer_load"),
         ("gst", r"global_store|global_atomic"), ("dsr", r"ds_read"), ("dsw", r"ds_write"), ("cmp", r"v_cmp"), ("cnd", r"v_cndmask")]


def main():
    path, name = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(name), l))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel") or lines[i].strip() == "s_endpgm")
    blocks, cur = [], {"label": "entry", "line": start + 1, "valu": 0, "marks": {}, "br": []}
    for i in range(start + 1, end + 1):
        l = lines[i].split(";")[0].strip()
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            blocks.append(cur)
            cur = {"label": m.group(1), "line": i + 1, "valu": 0, "marks": {}, "br": []}
            continue
        if not l or l.startswith("."):
            continue
        if l.startswith("v_"):
            cur["valu"] += 1
        for k, pat in MARKS:
            if re.search(pat, l):
                cur["marks"][k] = cur["marks"].get(k, 0) + 1
        m = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", l)
        if m:
            cur["br"].append(m.group(1))
    blocks.append(cur)
    order = {b["label"]: n for n, b in enumerate(blocks)}
    total = 0
    for n, b in enumerate(blocks):
        total += b["valu"]
        back = [t for t in b["br"] if order.get(t, 1 << 30) <= n]
        marks = " ".join(f"{k}={v}" for k, v in b["marks"].items())
        print(f"{b['label']:12s} L{b['line']:<6d} valu {b['valu']:4d}  {marks}{'  LOOP->' + ','.join(back) if back else ''}")
    print(f"total static VALU {total} in {len(blocks)} blocks")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Resource table of EVERY kernel of a build (not only the render kernels the spill gate counts):
tools/kernel_resources.py <objdir> [name filter ...] prints, per kernel whose demangled name holds
one of the filters, VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch bytes per lane, static LDS
bytes per workgroup and waves per SIMD, from the compiler's remarks (<objdir>/<unit>.res).  Two
tables of two trees diff line by line (profiles/radiance/resources.txt)."""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spill_gate import demangle  # noqa: E402

FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "VGPRs Spill": "vspill", "SGPRs Spill": "sspill",
          "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occ"}


def parse(text):
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([^:]+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = m.group(2)
    return rows


def main():
    objdir, filters = sys.argv[1], sys.argv[2:]
    rows = []
    for res in sorted(glob.glob(os.path.join(objdir, "*.res"))):
        rows += parse(open(res, errors="replace").read())
    for r, d in zip(rows, demangle([r["name"] for r in rows])):
        r["pretty"] = re.sub(r"\(.*\)$", "", d)
    rows = sorted((r for r in rows if not filters or any(f in r["pretty"] for f in filters)), key=lambda r: r["pretty"])
    print("# kernel vgpr agpr sgpr vspill sspill scratch lds occ (tools/kernel_resources.py)")
    for r in rows:
        print(r["pretty"], *[r.get(k) for k in ("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds", "occ")])
    return 0


if __name__ == "__main__":
    sys.exit(main())

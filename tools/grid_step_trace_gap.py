#!/usr/bin/env python
"""GPU idle time between two bench steps, from a rocprofv3 kernel trace: python tools/grid_step_trace_gap.py DIR

DIR holds the csv output of `rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 3 --warmup 1 [--engine-opts grid_fused=0]`.
A grid8 step ends with blend_normalize_kernel; the next step's U-Net starts with its first conv kernel.  Prints, for every step boundary, the interval
from the end of the normalise kernel to the start of the next conv kernel, and how much of it the small kernels in between (noise, gather, conditioning
rows, copies' kernels, embedding) occupy.  Tracing slows the host: the figure is indicative."""
import csv
import glob
import sys


def main(d):
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0]))
    rows.sort()
    ends = [i for i, r in enumerate(rows) if "blend_normalize_kernel" in r[2]]
    print(f"{len(rows)} kernel records, {len(ends)} steps")
    for i in ends:
        nxt = next((j for j in range(i + 1, len(rows)) if "conv" in rows[j][2]), None)
        if nxt is None:
            continue
        gap = (rows[nxt][0] - rows[i][1]) / 1e3
        busy = sum(rows[j][1] - rows[j][0] for j in range(i + 1, nxt)) / 1e3
        print(f"  normalise end -> first conv of the next step: {gap:9.1f} us, {nxt - i - 1} kernels in between busy for {busy:7.1f} us, idle {gap - busy:9.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])

"""The host round trip of the K x K eigensolve as the GPU sees it, from a rocprofv3 kernel trace of the headline run (the method
of tools/r06/restart_gaps.py pointed at bench.py): for every rotation launch, the time from the end of the cycle's closing
launch (k_lz_finish) to the start of the rotation, the kernels inside that window, and the merge kernels' own durations
(k_mg_*, csrc/merge_device.hip.hpp).  Also the per-kernel totals of the whole trace.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 20 --warmup 5
  python tools/device_merge_gaps.py DIR [fraction of the trace's tail to use, default 1/3: the timed windows]"""
import collections
import csv
import glob
import os
import re
import sys

import numpy as np

files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)
tail = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0 / 3.0
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), re.sub(r"[<(].*", "", r["Kernel_Name"]).split("::")[-1]))
rows.sort()
tot = collections.defaultdict(lambda: [0, 0.0])
for s, e, n in rows:
    tot[n][0] += 1; tot[n][1] += (e - s) / 1e3
span = (rows[-1][1] - rows[0][0]) / 1e3
busy_all = sum(v[1] for v in tot.values())
print("kernels %d, trace span %.1f ms, kernel time %.1f ms" % (len(rows), span / 1e3, busy_all / 1e3))
print("| kernel | calls | total ms | mean us | % of kernel time |\n|---|---|---|---|---|")
for n, (c, t) in sorted(tot.items(), key=lambda kv: -kv[1][1])[:14]:
    print("| %s | %d | %.2f | %.2f | %.1f |" % (n, c, t / 1e3, t / c, 100 * t / busy_all))

gaps, busy, inside, mg = [], [], collections.Counter(), collections.defaultdict(list)
first = int(len(rows) * (1.0 - tail))
for i, (s, e, n) in enumerate(rows):
    if i < first or "k_lz_rotate" not in n:
        continue
    j, inter, names = i - 1, 0.0, []
    while j >= 0 and i - j <= 12 and "k_lz_finish" not in rows[j][2]:
        inter += (rows[j][1] - rows[j][0]) / 1e3
        names.append(rows[j][2])
        j -= 1
    if j < 0 or "k_lz_finish" not in rows[j][2]:
        continue                                        # not a rotation behind a cycle (a second rotation of the same eigensolve)
    gaps.append((s - rows[j][1]) / 1e3); busy.append(inter)
    inside[" ".join(reversed(names))] += 1
    for q in range(j + 1, i):
        if "k_mg_" in rows[q][2]:
            mg[rows[q][2]].append((rows[q][1] - rows[q][0]) / 1e3)
    if any("k_mg_" in nm for nm in names):
        mg["first merge launch -> rotation start"].append((s - min(rows[q][0] for q in range(j + 1, i) if "k_mg_" in rows[q][2])) / 1e3)
g, b = np.array(gaps), np.array(busy)
print("\nrotations behind a closing launch in the last %.0f %% of the trace: %d" % (100 * tail, len(g)))
print("closing launch end -> rotation start: median %.1f us, 10 %% %.1f, 90 %% %.1f; kernel time inside: median %.1f us; idle: median %.1f us"
      % (np.median(g), np.percentile(g, 10), np.percentile(g, 90), np.median(b), np.median(g - b)))
for names, c in inside.most_common(4):
    print("  %5d x  [%s]" % (c, names))
for n, v in mg.items():
    print("  %-40s median %.2f us, 10 %% %.2f, 90 %% %.2f (%d)" % (n, np.median(v), np.percentile(v, 10), np.percentile(v, 90), len(v)))

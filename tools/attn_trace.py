"""Attention per layer and kernel time per step from a rocprofv3 kernel trace of `bench.py --towers pair` (serialized: one stream).
usage: python3 tools/attn_trace.py <*_kernel_trace.csv> [layers per step, default 12]
A layer's attention is the launches of attention_mfma* between two in_proj GEMMs: two (image, text) or the one pair launch; their
durations are summed per layer.  A step is `layers` consecutive layers; its kernel time is the sum of the durations of every
kernel from its first attention launch up to the next step's (a window one step long that starts inside the step)."""
import csv, statistics, sys

rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(sys.argv[1]))))
layers = int(sys.argv[2]) if len(sys.argv) > 2 else 12
groups, names = [], {}          # groups: [index of the first launch, summed ns, launches]
for i, (s, e, n) in enumerate(rows):
    if "attention_mfma" not in n:
        continue
    names[n] = names.get(n, 0) + 1
    if groups and all("attention_mfma" in rows[j][2] or "amax" in rows[j][2] for j in range(groups[-1][0], i)):
        groups[-1][1] += e - s; groups[-1][2] += 1
    else:
        groups.append([i, e - s, 1])
for n, c in sorted(names.items()):
    print(f"{c:6d} launches  {n[:110]}")
us = [g[1] / 1e3 for g in groups]
print(f"attention per layer: {len(groups)} layers, launches per layer {sorted(set(g[2] for g in groups))}: "
      f"median {statistics.median(us):.2f} us  min {min(us):.2f}  max {max(us):.2f}")
starts = [groups[k][0] for k in range(0, len(groups), layers)]
steps = [sum(e - s for s, e, _ in rows[a:b]) / 1e6 for a, b in zip(starts, starts[1:])]
print(f"kernel time per step: {len(steps)} windows: median {statistics.median(steps):.4f} ms  min {min(steps):.4f}  max {max(steps):.4f}")

#!/usr/bin/env python
"""What the K-Net's residual passes run beside, from a rocprofv3 --kernel-trace CSV of the pipelined bench.py:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 20 --warmup 6
    python tools/pass_overlap.py DIR/**/*kernel_trace.csv

The passes are the nhwc_act dispatches of the largest grid (the D-Net's are 50x smaller) or, where the trace has them, the
nhwc_act_lean dispatches.  For each pass: its duration, and the fraction of its interval during which a conv_wino_pc / conv2d_mfma
dispatch was running (those can only be the other stream's: a stream runs one kernel at a time) or any other kernel at all.
One row per position in the frame (the four passes in order), mean / min / max over the steady-state frames."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
rows.sort(key=lambda r: r["s"])
rows = [r for r in rows if r["s"] >= rows[0]["s"] + 0.5 * (rows[-1]["e"] - rows[0]["s"])]     # replayed frames only
grid = lambda r: int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)
lean = [r for r in rows if "nhwc_act_lean" in r["Kernel_Name"]]
fat = [r for r in rows if "nhwc_act_kernel" in r["Kernel_Name"]]
big = max(grid(r) for r in fat) if fat else 0
passes = lean or [r for r in fat if grid(r) == big]
convs = [r for r in rows if "conv_wino_pc_kernel" in r["Kernel_Name"] or "conv2d_mfma_kernel" in r["Kernel_Name"]]


def covered(p, others):
    """Fraction of p's interval covered by the union of the others' intervals."""
    iv = sorted((max(o["s"], p["s"]), min(o["e"], p["e"])) for o in others if o is not p and o["s"] < p["e"] and o["e"] > p["s"])
    tot, end = 0, p["s"]
    for s, e in iv:
        if e > end:
            tot += e - max(s, end)
            end = e
    return tot / float(p["e"] - p["s"])


# position in the frame: the passes come in groups of four, separated by the rest of the frame
groups, cur = [], []
for p in passes:
    if cur and p["s"] - cur[-1]["e"] > 8e6:          # > 8 ms since the last pass: a new frame
        groups.append(cur); cur = []
    cur.append(p)
groups.append(cur)
groups = [g for g in groups if len(g) == 4]
print("%d passes (%s, grid %d), %d whole frames" % (len(passes), "lean form" if lean else "fat form",
                                                       grid(passes[0]), len(groups)))
print("pass   duration us: mean   min   max    beside a 2-D conv: mean   min   max    beside any kernel: mean")
tot_d = 0.0
for k in range(4):
    ps = [g[k] for g in groups]
    d = [(p["e"] - p["s"]) / 1e3 for p in ps]
    c = [covered(p, convs) for p in ps]
    a = [covered(p, rows) for p in ps]
    tot_d += sum(d) / len(d)
    print("%4d   %17.1f %5.1f %5.1f    %23.2f  %4.2f  %4.2f    %23.2f" % (k, sum(d) / len(d), min(d), max(d), sum(c) / len(c), min(c), max(c),
                                                                   sum(a) / len(a)))
allp = [p for g in groups for p in g]
print("all    %17.1f (sum of the four means)   %17.2f %31.2f" % (tot_d, sum(covered(p, convs) for p in allp) / len(allp),
                                                              sum(covered(p, rows) for p in allp) / len(allp)))
# the frame: from one frame's first pass to the next one's
if len(groups) > 1:
    per = [(b[0]["s"] - a[0]["s"]) / 1e6 for a, b in zip(groups, groups[1:])]
    print("frame period (first pass to first pass): mean %.3f ms  min %.3f  max %.3f" % (sum(per) / len(per), min(per), max(per)))

# The other stream's 2-D convolutions by what they ran beside: for every conv dispatch, the kernel of the passes' stream that covers
# most of its interval ("alone" where none covers a tenth of it); mean duration per form and neighbour
stream = lambda r: (r.get("Queue_Id"), r.get("Stream_Id"))
main = stream(passes[0])
short = lambda n: n.replace("void ", "").replace("nrgbd::", "").split("(")[0][:60]
back = [r for r in rows if stream(r) == main]
table = {}
for cv in (r for r in convs if stream(r) != main):
    best, bn = 0.1 * (cv["e"] - cv["s"]), "alone"
    for o in back:
        if o["s"] >= cv["e"]:
            break
        ov = min(o["e"], cv["e"]) - max(o["s"], cv["s"])
        if ov > best:
            best, bn = ov, short(o["Kernel_Name"]).split("<")[0]
    t = table.setdefault(("%s grid %d" % (short(cv["Kernel_Name"]), grid(cv)), bn), [0, 0.0])
    t[0] += 1
    t[1] += (cv["e"] - cv["s"]) / 1e3
print("\nthe other stream's 2-D convolutions, by the kernel of the passes' stream they ran beside (count, mean us):")
for name in sorted({k[0] for k in table}, key=lambda n: -sum(v[1] for k, v in table.items() if k[0] == n)):
    cells = sorted(((k[1], v) for k, v in table.items() if k[0] == name), key=lambda kv: -kv[1][1])
    print("  %-78s %s" % (name, "   ".join("%s %d x %.1f" % (b, v[0], v[1] / v[0]) for b, v in cells[:6])))

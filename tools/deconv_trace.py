"""The R-Net's two transposed convolutions and their neighbours in a `rocprofv3 --kernel-trace` CSV of bench.py (profiles/deconv_wino.txt):
per launch form (kernel, grid) of the transposed convolutions the count and the mean / min / max duration, and the same for the kernel
launched before and behind each of them on its queue.  (The feature CNN's stride-2 layer runs on the direct form's kernel too and is
listed with it: grid 245760 at config B, behind space_to_depth2.)

    python tools/deconv_trace.py DIR/**/*kernel_trace.csv [launches of the timed frames to keep, counted from the end: default all]"""
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
rows.sort(key=lambda r: r["s"])
grid = lambda r: int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)
short = lambda n: re.sub(r"^void |nrgbd::|\(.*$", "", n)
form = lambda r: "%s grid %d" % (short(r["Kernel_Name"]), grid(r))
# the direct form: conv2d_mfma_kernel<64, 1, false, 4, 0>; the Winograd deconv form: conv_wino_pc_kernel<1, 1, false, false, 2, ...>
is_deconv = lambda r: re.search(r"conv2d_mfma_kernel<64, 1, false, 4, 0>|conv_wino_pc_kernel<1, 1, false, false, 2,", r["Kernel_Name"]) is not None
queues = {}
for r in rows:
    queues.setdefault((r.get("Queue_Id"), r.get("Stream_Id")), []).append(r)
table = {}
for q in queues.values():
    for i, r in enumerate(q):
        if not is_deconv(r):
            continue
        # both layers of the Winograd form run on one persistent grid: the kernel in front tells them apart (conv0_1 is the
        # 64-column form, conv1_1's last launch the 32-column HALF form)
        key = form(r) + (" after " + short(q[i - 1]["Kernel_Name"]).split("(")[0] if i else "")
        for role, o in (("", r), ("  before: ", q[i - 1] if i else None), ("  behind: ", q[i + 1] if i + 1 < len(q) else None)):
            if o is not None:
                table.setdefault((key, role + (form(o) if role else "")), []).append((o["e"] - o["s"]) / 1e3)
keep = int(sys.argv[2]) if len(sys.argv) > 2 else 0
print("%-150s %6s %9s %9s %9s" % ("launch", "count", "mean us", "min", "max"))
for (key, role), d in sorted(table.items()):
    d = d[-keep:] if keep else d
    print("%-150s %6d %9.1f %9.1f %9.1f" % ((key if not role else role)[:150], len(d), sum(d) / len(d), min(d), max(d)))

#!/usr/bin/env python
"""Reduce rocprofv3's ``*kernel_stats.csv`` of a ``tests/bench_drn.py --workload source_only`` run to the committed text summary.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o drn -- python tests/bench_drn.py --workload source_only --steps 3 --warmup 2
    python profiles/drn_kernel_stats.py OUT profiles/drn_source_only_b8_kernel_stats.txt

Besides the per-kernel table it prints the share of the DRN head's own convolution kernels (uda_clr_amd/csrc/drn_head.hip:
stem7s1_* = layer0, conv3n_*<16, ..> / <32, 16, 1> = layer1 - layer2 forward + backward, conv3n_*<64, 64, ..> = layer3.0.conv2 and the weight gradients of layer3.1 / layer3.2).
The BatchNorm passes of the head layers run on the kernels every layer uses and cannot be told apart by name.
"""
import csv
import glob
import os
import re
import sys


def main(src, dst, title):
    paths = glob.glob(os.path.join(src, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_stats.csv under " + src)
    rows = []
    with open(paths[0]) as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]), int(float(r["TotalDurationNs"]))))
    rows.sort(key=lambda r: -r[2])
    total = sum(r[2] for r in rows)

    def short(n):
        return re.sub(r"\(.*", "", n)[:72]
    head = {"layer0 (stem7s1_*)": 0, "layer1 - layer2 (conv3n_* at 16 / 32 channels)": 0, "layer3 conv2 at 64 -> 64 (conv3n_*<64, 64, .>)": 0}
    for n, c, t in rows:
        if "stem7s1" in n:
            head["layer0 (stem7s1_*)"] += t
        elif "conv3n" in n:
            head["layer3 conv2 at 64 -> 64 (conv3n_*<64, 64, .>)" if re.search(r"<64, ?64", n) else "layer1 - layer2 (conv3n_* at 16 / 32 channels)"] += t
    with open(dst, "w") as f:
        f.write(title + "\n")
        f.write("%-72s %6s %14s %10s %6s\n" % ("kernel", "calls", "total_ns", "avg_ns", "pct"))
        for n, c, t in rows[:40]:
            f.write("%-72s %6d %14d %10d %5.1f%%\n" % (short(n), c, t, t // max(c, 1), 100.0 * t / total))
        rest = rows[40:]
        f.write("%-72s %6d %14d %10s %5.1f%%\n" % ("(%d more kernels)" % len(rest), sum(r[1] for r in rest), sum(r[2] for r in rest), "",
                                                   100.0 * sum(r[2] for r in rest) / total))
        f.write("%-72s %6d %14d\n\n" % ("all kernels", sum(r[1] for r in rows), total))
        f.write("convolution kernels of the DRN head, share of all kernel time:\n")
        for k, t in head.items():
            f.write("  %-52s %12d ns  %5.2f%%\n" % (k, t, 100.0 * t / total))
        f.write("  %-52s %12d ns  %5.2f%%\n" % ("sum", sum(head.values()), 100.0 * sum(head.values()) / total))
    print(open(dst).read())


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else
         "rocprofv3 --kernel-trace --stats, python tests/bench_drn.py --workload source_only --steps 3 --warmup 2\n"
         "(DeepLab drn, 512^2, B = 8, MI355X; 5 steps traced incl. warm-up; durations in ns)")

"""Kernel statistics of the timed cycles of one tools/bench_multirhs.py run under `rocprofv3 --kernel-trace` (SQLite
output, the `kernels` view): the launches after the last idle gap of the trace (`--pause-ms`), i.e. the timed cycles of the
last NV the run measured, per kernel symbol and grid size.

    python tools/multirhs_trace_stats.py <results.db> <cycles> <out.csv>
"""
import csv
import sqlite3
import sys


def main():
    db, cycles, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    rows = list(sqlite3.connect(db).execute("select name, grid_x, start, end from kernels order by start"))
    # the last gap between the end of one launch and the start of the next that is longer than 100 ms
    cut = 0
    last_end = rows[0][3]
    for i in range(1, len(rows)):
        if rows[i][2] - last_end > 100_000_000:
            cut = i
        last_end = max(last_end, rows[i][3])
    timed = rows[cut:]
    stats = {}
    for name, grid, start, end in timed:
        key = (name.split("(")[0][:120], grid)
        c = stats.setdefault(key, [0, 0])
        c[0] += 1
        c[1] += end - start
    busy = sum(v[1] for v in stats.values())
    span = timed[-1][3] - timed[0][2]
    with open(out, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["kernel", "grid_x", "launches_per_cycle", "us_per_cycle", "percent_of_kernel_time"])
        for (name, grid), (calls, ns) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
            w.writerow([name, grid, round(calls / cycles, 2), round(ns / cycles / 1e3, 2), round(100.0 * ns / busy, 2)])
    print("launches %d over %d cycles: %.3f ms of kernels and %.3f ms wall per cycle" % (len(timed), cycles, busy / cycles / 1e6, span / cycles / 1e6))


if __name__ == "__main__":
    main()

"""Per-kernel summary of a kernel trace of scratch/hubert_time.py:

    rocprofv3 --kernel-trace --stats -d TRACE_DIR -o hub -- python scratch/hubert_time.py --only native --calls 5
    python scratch/hubert_trace_summary.py TRACE_DIR/.../hub_results.db

Prints the total and median device time per (kernel, grid), sorted by total (profiles/r05_hubert_kernel_stats.txt)."""
import collections
import re
import sqlite3
import sys


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rows = sqlite3.connect(sys.argv[1]).execute("select name, duration, grid_x, grid_y, grid_z from kernels order by start").fetchall()
    agg = collections.defaultdict(list)
    for name, dur, gx, gy, gz in rows:
        agg[(re.sub(r"\(.*", "", name)[:70], gx, gy, gz)].append(dur / 1e3)
    print("total_us calls median_us kernel grid")
    for key in sorted(agg, key=lambda k: -sum(agg[k]))[:40]:
        v = sorted(agg[key])
        print(f"{sum(v):10.0f} {len(v):5d} {v[len(v) // 2]:9.1f}  {key[0]}  grid={key[1:]}")


if __name__ == "__main__":
    main()

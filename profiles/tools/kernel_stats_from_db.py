"""Dev tool: the per-kernel summary of a `rocprofv3 --kernel-trace --stats` run, aggregated from the run's trace database, in the column layout of the
rXX_kernel_stats.csv files.  usage: python profiles/tools/kernel_stats_from_db.py <results.db> <out.csv>"""
import csv
import sqlite3
import statistics
import sys

db = sqlite3.connect(sys.argv[1])
rows = db.execute("select s.kernel_name, d.end - d.start from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on s.id = d.kernel_id").fetchall()
by = {}
for name, ns in rows:
    by.setdefault(name, []).append(ns)
total = sum(sum(v) for v in by.values())
with open(sys.argv[2], "w", newline="") as f:
    w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
    w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
    for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        w.writerow([name, len(v), sum(v), round(sum(v) / len(v), 6), round(100.0 * sum(v) / total, 4), min(v), max(v), round(statistics.pstdev(v), 6)])

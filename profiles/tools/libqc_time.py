#!/usr/bin/env python3
"""Timing of the library profile (mirp_libqc_reads) on trim_time.py's seeded FASTQ library of about 30 M raw reads, beside the trim
(mirp_trim_reads) of the same file in the same session.

    python profiles/tools/libqc_time.py [--reads 30000000] [--file /tmp/trim_30M.fastq] [--out build/libqc_time/libqc_time.json] [--sample S]
                                        [--trim] [--numpy-reads N]

The file is trim_time.py's (made here when it is missing): 51-nt reads of an 18-26-nt insert, the Illumina small-RNA adapter with 1 % substitutions
and a random tail, 5 % dimers.  The call runs twice (the first loads the code objects); the second is reported with its phase breakdown and what
it found.  --trim: the trim's call with the found adapter follows, twice as well, for the comparison.  The numpy restatement of the k-mer table and
the walk (tests/libqc_restatement.py) runs on the first --numpy-reads reads (0: skipped) and must find the same adapter when the sample is the
same.  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats` (with --numpy-reads 0); --kernel-stats turns them into
bytes moved (what the algorithm has to read and write, counted from the sizes of the run) over kernel time, against 8 TB/s."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trim_time import ADAPTER, HBM, READ_LEN, make_file  # noqa: E402

PHASES = ("upload", "split", "records", "kmers_adapter", "trim", "tables")
RECORD = 12 + 2 * READ_LEN + 4            # bytes of one FASTQ record of the file


def kernel_bytes(s):
    """Bytes each kernel has to move at the sizes of a run: N text bytes, L lines, R reads, S sampled reads, C distinct 12-mers counted."""
    N, L, R, S = s["bytes"], s["lines"], s["reads"], s["sampled"]
    tiles = N / 4096
    table = 4 * (1 << 24)
    return {
        "reads_count_kernel": N + 4 * tiles,
        "reads_starts_kernel": N + 8 * tiles + 8 * L,
        "trim_fastq_records_kernel": 8 * L + N + R * (8 + 4 + 8 + 8 + 4),
        "libqc_kmer_kernel": S * (8 + 4) + S * min(READ_LEN, 64),             # read records and the first 64 bases; the counters stay in cache
        "libqc_seed_kernel": table,
        "libqc_walk_kernel": 0,
        "trim_reads_kernel": R * (8 + 4 + 8 + 4) + 2 * READ_LEN * R,
        "libqc_cycles_kernel": R * (8 + 4 + 8) + 2 * READ_LEN * R,             # read records, the sequence and quality bytes
        "libqc_insert_kernel": R * (8 + 4 + 4) + R,                            # read records, the final lengths, the first base
    }


def report_kernel_stats(stats_csv, sizes):
    by = kernel_bytes(sizes)
    rows = []
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            tot_ns = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
            calls = int(float(r.get("Calls") or 1))
            short = next((k for k in by if k in name), None)
            rows.append((name[:70], calls, tot_ns / calls / 1e6, short))
    for name, calls, ms, short in sorted(rows, key=lambda x: -x[2] * x[1]):
        if short and by[short]:
            bw = by[short] / (ms * 1e-3)
            print("%-70s %3d calls  %8.3f ms/call  %7.1f GB/s  %5.1f %% of 8 TB/s" % (name, calls, ms, bw / 1e9, 100 * bw / HBM))
        else:
            print("%-70s %3d calls  %8.3f ms/call" % (name, calls, ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30000000)
    ap.add_argument("--file", default="/tmp/trim_30M.fastq")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "libqc_time", "libqc_time.json"))
    ap.add_argument("--sample", type=int, default=1 << 20)
    ap.add_argument("--trim", action="store_true")
    ap.add_argument("--numpy-reads", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--sizes")
    a = ap.parse_args()
    if a.kernel_stats:
        report_kernel_stats(a.kernel_stats, json.load(open(a.sizes)))
        return
    from mir_prefer_amd import capi
    if not os.path.exists(a.file) or os.path.getsize(a.file) != a.reads * RECORD:
        t = time.time()
        make_file(a.file, a.reads, a.seed)
        print("made %s (%d bytes) in %.1f s" % (a.file, os.path.getsize(a.file), time.time() - t), flush=True)
    ctx = capi.Context(0)
    res = None
    for run in range(2):
        t0 = time.time()
        with open(a.file, "rb") as f:
            data = f.read()
        t_read = time.time() - t0
        res = ctx.libqc_reads(data, a.file, sample=a.sample)
        wall = time.time() - t0
        print("libqc run %d: wall %.3f s (file read %.3f s), phases %s" % (run, wall, t_read, ["%.4f" % x for x in res["seconds"]]), flush=True)
    found = {k: res[k] for k in ("adapter", "status", "seed", "seed_count", "min_count", "left_steps", "left_stop")}
    counts = {k: res[k] for k in capi.LIBQC_STATS}
    print("found %s, counts %s" % (found, counts), flush=True)
    assert res["adapter"].startswith(ADAPTER.decode()) or ADAPTER.decode().startswith(res["adapter"]), "the planted adapter was not found"
    sizes = {"bytes": len(data), "lines": 4 * res["reads"], "reads": res["reads"], "sampled": res["sampled"]}
    rec = {"reads": res["reads"], "bytes": len(data), "wall_s": wall, "file_read_s": t_read, "phases_s": dict(zip(PHASES, res["seconds"])), "found": found,
           "counts": counts, "sizes": sizes}
    if a.trim:
        out = a.file + ".trimmed.fa"
        for run in range(2):
            t0 = time.time()
            with open(a.file, "rb") as f:
                data = f.read()
            t_read = time.time() - t0
            tr = ctx.trim_reads(data, a.file, out, adapter=res["adapter"], error_permille=100, overlap=3, quality=20, min_length=18)
            t_wall = time.time() - t0
            print("trim run %d: wall %.3f s (file read %.3f s), phases %s" % (run, t_wall, t_read, ["%.4f" % x for x in tr["seconds"]]), flush=True)
        rec["trim"] = {"wall_s": t_wall, "file_read_s": t_read,
                       "phases_s": dict(zip(("upload", "split", "records", "trim", "emit_download", "write"), tr["seconds"]))}
    ctx.close()
    if a.numpy_reads:
        from tests import libqc_restatement as lr
        n = min(a.numpy_reads, res["reads"])
        reads = data[:n * RECORD].split(b"\n")[1::4]
        del data
        t = time.time()
        want = lr.find_adapter(lr.table_numpy(reads, a.sample), n)
        rec["numpy_s"] = time.time() - t
        rec["numpy_reads"] = n
        print("numpy restatement: table and walk of %d reads in %.2f s: %s" % (n, rec["numpy_s"], want["adapter"]))
        if min(n, a.sample) == res["sampled"]:
            assert want == found, (want, found)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the read trimming (mirp_trim_reads) on a seeded FASTQ library of about 30 M raw reads, against the numpy restatement of
tests/test_trim_cpu.py on the same host.

    python profiles/tools/trim_time.py [--reads 30000000] [--file /tmp/trim_30M.fastq] [--out build/trim_time/trim_time.json] [--numpy-reads N]

The file: 51-nt reads, each an 18-26-nt insert drawn Zipf(1.2) from a pool of 2 M, then the Illumina small-RNA adapter TGGAATTCTCGGGTGCCAAGG
with 1 % substitutions, then a random tail; 5 % adapter dimers; qualities that fall along the read; headers `@r<9 digits>`.  The call runs twice
(the first loads the code objects); the second is reported with its phase breakdown.  The numpy restatement runs on the first --numpy-reads reads
of the same file (0: skipped); the whole file does not fit its per-read matrices.  Kernel times come from a run of its own under
`rocprofv3 --kernel-trace --stats` (with --numpy-reads 0); --kernel-stats turns them into bytes moved (what the algorithm has to read and write,
counted from the sizes of the run) over kernel time, against 8 TB/s."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM = 8.0e12
ADAPTER = b"TGGAATTCTCGGGTGCCAAGG"
READ_LEN = 51


def make_file(path, n_reads, seed):
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    n_pool = 2000000
    pool = acgt[rng.randint(0, 4, size=(n_pool, 26))]
    pool_len = rng.randint(18, 27, size=n_pool)
    ad = np.frombuffer(ADAPTER, dtype=np.uint8)
    qual_base = np.clip(40 - np.arange(READ_LEN) * 30 // READ_LEN, 2, 40)
    chunk = 1000000
    with open(path, "wb") as f:
        for a in range(0, n_reads, chunk):
            n = min(chunk, n_reads - a)
            idx = np.minimum(rng.zipf(1.2, size=n) - 1, n_pool - 1)
            ln = pool_len[idx]
            ln[rng.rand(n) < 0.05] = 0                                    # adapter dimers
            seq = acgt[rng.randint(0, 4, size=(n, READ_LEN))]             # the random tail
            cols = np.arange(READ_LEN)[None, :]
            ins = cols < ln[:, None]
            seq[:, :26] = np.where(ins[:, :26], pool[idx], seq[:, :26])
            k = cols - ln[:, None]
            in_ad = (k >= 0) & (k < len(ad))
            adb = ad[np.clip(k, 0, len(ad) - 1)]
            err = in_ad & (rng.rand(n, READ_LEN) < 0.01)
            adb = np.where(err, acgt[rng.randint(0, 4, size=(n, READ_LEN))], adb)
            seq = np.where(in_ad, adb, seq)
            qual = np.clip(qual_base[None, :] + rng.randint(-5, 6, size=(n, READ_LEN)), 2, 41).astype(np.uint8) + 33
            hdr = np.frombuffer(b"".join(b"@r%09d\n" % (a + j) for j in range(n)), dtype=np.uint8).reshape(n, 12)
            nl = np.full((n, 1), 10, np.uint8)
            plus = np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0)
            f.write(np.concatenate([hdr, seq, nl, plus, qual, nl], axis=1).tobytes())


def kernel_bytes(s):
    """Bytes each kernel has to move at the sizes of a run: N text bytes, L lines, R reads, T output bytes."""
    N, L, R, T = s["bytes"], s["lines"], s["reads"], s["out_bytes"]
    tiles = N / 4096
    return {
        "reads_count_kernel": N + 4 * tiles,
        "reads_starts_kernel": N + 8 * tiles + 8 * L,
        "trim_fastq_records_kernel": 8 * L + N + R * (8 + 4 + 8 + 8 + 4),     # line starts, the header / sequence / quality bytes, the read records
        "trim_reads_kernel": R * (8 + 4 + 8 + 4) + 2 * READ_LEN * R,           # read records, the sequence and quality slab, the final lengths
        "trim_size_kernel": R * 12,
        "trim_emit_kernel": R * (8 + 4 + 8 + 4 + 8) + 2 * T,                   # records, the name and read bytes read, the text written
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
        if short:
            bw = by[short] / (ms * 1e-3)
            print("%-70s %3d calls  %8.3f ms/call  %7.1f GB/s  %5.1f %% of 8 TB/s" % (name, calls, ms, bw / 1e9, 100 * bw / HBM))
        else:
            print("%-70s %3d calls  %8.3f ms/call" % (name, calls, ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30000000)
    ap.add_argument("--file", default="/tmp/trim_30M.fastq")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "trim_time", "trim_time.json"))
    ap.add_argument("--numpy-reads", type=int, default=2000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--sizes")
    a = ap.parse_args()
    if a.kernel_stats:
        report_kernel_stats(a.kernel_stats, json.load(open(a.sizes)))
        return
    from mir_prefer_amd import capi
    if not os.path.exists(a.file) or os.path.getsize(a.file) != a.reads * (12 + 2 * READ_LEN + 4):
        t = time.time()
        make_file(a.file, a.reads, a.seed)
        print("made %s (%d bytes) in %.1f s" % (a.file, os.path.getsize(a.file), time.time() - t), flush=True)
    out = a.file + ".trimmed.fa"
    ctx = capi.Context(0)
    kw = dict(adapter=ADAPTER.decode(), error_permille=100, overlap=3, quality=20, min_length=18)
    res = None
    for run in range(2):
        t0 = time.time()
        with open(a.file, "rb") as f:
            data = f.read()
        t_read = time.time() - t0
        res = ctx.trim_reads(data, a.file, out, **kw)
        wall = time.time() - t0
        print("run %d: wall %.3f s (file read %.3f s), phases %s" % (run, wall, t_read, ["%.4f" % x for x in res["seconds"]]), flush=True)
    ctx.close()
    sizes = {"bytes": len(data), "lines": 4 * res["reads"], "reads": res["reads"], "out_bytes": os.path.getsize(out)}
    rec = {"reads": res["reads"], "bytes": len(data), "wall_s": wall, "file_read_s": t_read,
           "phases_s": dict(zip(("upload", "split", "records", "trim", "emit_download", "write"), res["seconds"])),
           "counts": {k: res[k] for k in capi.TRIM_STATS}, "sizes": sizes}
    del data
    if a.numpy_reads:
        from tests.test_trim_cpu import restate_trim_numpy
        with open(a.file, "rb") as f:
            part = f.read(a.numpy_reads * (12 + 2 * READ_LEN + 4))
        t = time.time()
        restate_trim_numpy(part, adapter=ADAPTER, e_pm=100, overlap=3, q=20, min_len=18)
        rec["numpy_s"] = time.time() - t
        rec["numpy_reads"] = a.numpy_reads
        print("numpy restatement: %d reads in %.2f s (%.2f s per M reads)" % (a.numpy_reads, rec["numpy_s"], rec["numpy_s"] / a.numpy_reads * 1e6))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

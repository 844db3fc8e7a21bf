#!/usr/bin/env python3
"""Timing of the read collapse (mirp_collapse_reads) on a seeded library of about 30 M reads, against the dict restatement of
scripts/process-reads-fasta.py:60-80 on the same file and host.

    python profiles/tools/collapse_time.py [--reads 30000000] [--out build/collapse_time/collapse_time.json] [--no-dict]
    python profiles/tools/collapse_time.py --kernel-stats <rocprofv3 kernel_stats.csv> --sizes <json of a run>   (bytes over time per kernel)

The file: FASTA, a header `>r<9 digits>` per read; 80 % of the reads drawn Zipf(1.2) from a pool of 2 M distinct 18-26-nt reads, 20 % singletons.
The call runs twice (the first loads the code objects); the second is reported with its phase breakdown.  Kernel times come from a run of its own
under `rocprofv3 --kernel-trace --stats` (with --no-dict); --kernel-stats turns them into bytes moved (what the algorithm has to read and write,
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


def make_file(path, n_reads, seed):
    rng = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    n_pool = 2000000
    pool = acgt[rng.randint(0, 4, size=(n_pool, 26))]
    pool_len = rng.randint(18, 27, size=n_pool)
    chunk = 2000000
    with open(path, "wb") as f:
        for a in range(0, n_reads, chunk):
            n = min(chunk, n_reads - a)
            single = rng.rand(n) < 0.2
            idx = np.minimum(rng.zipf(1.2, size=n) - 1, n_pool - 1)
            seq = pool[idx].copy()
            ln = pool_len[idx].copy()
            ns = int(single.sum())
            seq[single] = acgt[rng.randint(0, 4, size=(ns, 26))]
            ln[single] = rng.randint(18, 27, size=ns)
            hdr = np.frombuffer(b"".join(b">r%09d\n" % (a + k) for k in range(n)), dtype=np.uint8).reshape(n, 12)
            body = np.concatenate([seq, np.zeros((n, 1), dtype=np.uint8)], axis=1)
            body[np.arange(n), ln] = ord("\n")
            full = np.concatenate([hdr, body], axis=1)
            mask = np.concatenate([np.ones((n, 12), dtype=bool), np.arange(27)[None, :] <= ln[:, None]], axis=1)
            f.write(full[mask].tobytes())


def dict_restatement(path, prefix, out_path):
    t = time.time()
    d = {}
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                continue
            key = line.strip()
            if key in d:
                d[key] += 1
            else:
                d[key] = 1
    with open(out_path, "w") as o:
        for cnt, r in enumerate(d):
            o.write(">" + prefix + "_r" + str(cnt) + "_x" + str(d[r]) + "\n")
            o.write(r + "\n")
    return time.time() - t, len(d)


def kernel_bytes(s):
    """Bytes each kernel has to move at the sizes of a run: N text bytes, L lines, R reads of mean length m, U distinct, T output bytes."""
    N, L, R, U, T, m = s["bytes"], s["lines"], s["reads"], s["unique"], s["out_bytes"], s["mean_read_len"]
    tiles = N / 4096
    return {
        "reads_count_kernel": N + 4 * tiles,
        "reads_starts_kernel": N + 8 * tiles + 8 * L,
        "reads_flag_kernel": 8 * L + L + 4 * L,
        "reads_hash_kernel": 4 * L + 16 * R + 8 * R + R * (m + 2) + 16 * R + 16 * R,
        "sort_hist_kernel": 8 * 16 * R,
        "sort_scatter_kernel": 8 * 32 * R,
        "reads_runhead_kernel": 16 * R + 4 * R,
        "reads_runfirst_kernel": 4 * R + 8 * R + 8 * U,
        "reads_verify_kernel": R * (4 + 8 + 8 + 16 + 16 + 16 + 2 * m),
        "reads_tally_kernel": R * (16 + 4 + 8 + 8 + 4 + 4) + U * (8 + 8),
        "reads_size_kernel": R * (4 + 8 + 4 + 16 + 4),
        "reads_emit_kernel": R * 4 + U * (8 + 4 + 16 + 8 + m) + T,
    }


def kernel_report(stats_csv, sizes):
    want = kernel_bytes(sizes)
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            key = next((k for k in want if k in name), "excl_scan" if "excl_scan" in name else None)
            if key is None:
                continue
            rows.setdefault(key, [0, 0.0])
            rows[key][0] += int(r["Calls"])
            rows[key][1] += float(r["TotalDurationNs"]) * 1e-9 / 2      # two collapse calls per run (warm-up + timed)
    out = []
    for k, (calls, sec) in sorted(rows.items(), key=lambda x: -x[1][1]):
        b = want.get(k)
        out.append({"kernel": k, "calls_per_run": calls // 2, "ms": round(sec * 1e3, 3), "bytes": b,
                    "TB_s": round(b / sec / 1e12, 2) if b else None, "frac_of_8TBs": round(b / sec / HBM, 3) if b else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=30000000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "collapse_time"))
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "collapse_time", "collapse_time.json"))
    ap.add_argument("--no-dict", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--sizes")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_report(a.kernel_stats, json.load(open(a.sizes))["sizes"]), indent=1))
        return
    from mir_prefer_amd import capi
    os.makedirs(a.dir, exist_ok=True)
    path = os.path.join(a.dir, "lib.fa")
    t = time.time()
    make_file(path, a.reads, a.seed)
    gen_s = time.time() - t
    ctx = capi.Context(0)
    runs = []
    for _ in range(2):
        t = time.time()
        res = ctx.collapse_reads(path, "lib", path + ".processed")
        runs.append((time.time() - t, res))
    wall, res = runs[-1]
    out_bytes = os.path.getsize(path + ".processed")
    n_bytes = os.path.getsize(path)
    ctx.close()
    rep = {"reads": a.reads, "file_bytes": n_bytes, "generate_s": round(gen_s, 2), "first_call_s": round(runs[0][0], 4), "call_wall_s": round(wall, 4),
           "phases_s": dict(zip(["read_upload", "split", "hash_sort", "verify_rank", "emit_download", "write"], [round(x, 4) for x in res["seconds"]])),
           "n_reads": res["n_reads"], "n_unique": res["n_unique"], "collisions": res["collisions"],
           "sizes": {"bytes": n_bytes, "lines": 2 * res["n_reads"], "reads": res["n_reads"], "unique": res["n_unique"], "out_bytes": out_bytes,
                     "mean_read_len": 22.0}}
    if not a.no_dict:
        ds, nd = dict_restatement(path, "lib", path + ".dict")
        same = open(path + ".dict", "rb").read() == open(path + ".processed", "rb").read()
        rep.update({"dict_s": round(ds, 3), "dict_unique": nd, "outputs_identical": same, "speedup_vs_dict": round(ds / wall, 1)})
    for f in (path, path + ".processed", path + ".dict"):
        if os.path.exists(f):
            os.unlink(f)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()

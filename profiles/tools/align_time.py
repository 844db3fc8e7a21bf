#!/usr/bin/env python3
"""Timing of the read alignment (mirp_align_index / mirp_align_reads) on a seeded 120 Mb genome and 6.7 M distinct 18-26-nt reads, the index build
on a 2 Gb genome, and the searchsorted restatement of -v 0 (tests/test_align_cpu.py) on the same input and host.

    python profiles/tools/align_time.py [--genome-mb 120] [--reads 6700000] [--big-gb 2] [--no-restate] [--out build/align_time/align_time.json]
    python profiles/tools/align_time.py --kernel-stats <rocprofv3 kernel_stats.csv>      (kernel table: calls, total ms, share)
    python profiles/tools/align_time.py --tail 4 [--tail-min 16,12] [--repeat 5] --big-gb 0 --no-restate      (align --tail, DESIGN.md §12 "Tails")

Genome: random bases in 8 contigs, 2,000 segments of 1-5 kb copied to random places (repeats), 200 runs of 100 N.  Reads: half drawn from the
genome on both strands with 0 or 1 substitution (half each), half random; duplicates removed.  Every timed call runs after a first call of the same
kind (code objects loaded).  With --tail T a second read file is made from the same genome: a quarter of the reads (half of the random half) are
drawn from the genome on both strands with 1-4 appended U or A; the -v 0 -k 20 call is then timed --repeat times without and with --tail T on both
files (the spread of the repeated calls is what a difference between two builds is judged against).  Kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats` (with --no-restate --big-gb 0)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_genome(path, total, seed, n_contigs=8, repeats=True):
    rng = np.random.RandomState(seed)
    g = rng.randint(0, 4, size=total).astype(np.uint8)
    if repeats:
        for _ in range(2000):
            n = int(rng.randint(1000, 5001))
            a, b = int(rng.randint(0, total - n)), int(rng.randint(0, total - n))
            g[b:b + n] = g[a:a + n]
    text = ACGT[g]
    if repeats:
        for _ in range(200):
            a = int(rng.randint(0, total - 100))
            text[a:a + 100] = ord("N")
            g[a:a + 100] = 4
    cuts = np.linspace(0, total, n_contigs + 1).astype(np.int64)
    with open(path, "wb") as f:
        for c in range(n_contigs):
            f.write(b">chr%d\n" % (c + 1))
            seg = text[cuts[c]:cuts[c + 1]]
            w = 100
            full = len(seg) // w * w
            body = np.concatenate([seg[:full].reshape(-1, w), np.full((full // w, 1), 10, np.uint8)], axis=1)
            f.write(body.tobytes())
            if len(seg) > full:
                f.write(seg[full:].tobytes() + b"\n")
    return g


def make_reads(path, g, n_reads, seed, tailed=False):
    """tailed: the first half of the random half is drawn from the genome as well, exact, and its last 1-4 letters (as sequenced) are U or A."""
    rng = np.random.RandomState(seed)
    n = int(n_reads * 1.02)
    ln = rng.randint(18, 27, size=n)
    from_g = np.arange(n) < n // 2
    tail_g = (np.arange(n) >= n // 2) & (np.arange(n) < n // 2 + n // 4) if tailed else np.zeros(n, dtype=bool)
    tl = rng.randint(1, 5, size=n)
    if tailed:
        ln_t = np.where(tail_g, ln - tl, ln)        # the templated part of a tailed read; the strand flip below is that of this part
    seq = rng.randint(0, 4, size=(n, 26)).astype(np.uint8)
    off = rng.randint(0, len(g) - 26, size=int(from_g.sum()))
    seq[from_g] = np.minimum(g[off[:, None] + np.arange(26)[None, :]], 3)
    rc = from_g & (rng.rand(n) < 0.5)
    lr = ln
    if tailed:
        off_t = rng.randint(0, len(g) - 26, size=int(tail_g.sum()))
        seq[tail_g] = np.minimum(g[off_t[:, None] + np.arange(26)[None, :]], 3)
        rc = rc | (tail_g & (rng.rand(n) < 0.5))
        lr = ln_t
    # reverse complement of the first lr bases
    idx = lr[rc, None] - 1 - np.arange(26)[None, :]
    rows = seq[rc]
    seq[rc] = np.where(idx >= 0, 3 - np.take_along_axis(rows, np.maximum(idx, 0), axis=1), 0)
    if tailed:
        letter = np.where(rng.rand(n) < 0.7, 3, 0).astype(np.uint8)          # U more often than A
        col = np.arange(26)[None, :]
        in_tail = tail_g[:, None] & (col >= ln_t[:, None]) & (col < ln[:, None])
        seq[in_tail] = np.broadcast_to(letter[:, None], seq.shape)[in_tail]
    sub = from_g & (rng.rand(n) < 0.5)
    pos = (rng.rand(n) * ln).astype(np.int64)
    seq[sub, pos[sub]] = (seq[sub, pos[sub]] + 1 + rng.randint(0, 3, size=int(sub.sum()))) % 4
    seq[np.arange(26)[None, :] >= ln[:, None]] = 0
    key = np.zeros(n, dtype=np.uint64)
    for i in range(26):
        key = key * np.uint64(4) + seq[:, i].astype(np.uint64)
    key = key * np.uint64(32) + ln.astype(np.uint64)
    _, first = np.unique(key, return_index=True)
    keep = np.sort(first)[:n_reads]
    seq, ln = seq[keep], ln[keep]
    with open(path, "wb") as f:
        for a in range(0, len(keep), 1_000_000):
            b = min(a + 1_000_000, len(keep))
            lines = [b">S_r%d_x1\n%s\n" % (a + k, ACGT[seq[a + k, :ln[a + k]]].tobytes()) for k in range(b - a)]
            f.write(b"".join(lines))
    return len(keep)


def kernel_table(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        out.append({"kernel": r["Name"].split("(")[0][:80], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                    "share": float(r["TotalDurationNs"]) / tot})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=int, default=120)
    ap.add_argument("--reads", type=int, default=6_700_000)
    ap.add_argument("--big-gb", type=float, default=2.0)
    ap.add_argument("--no-restate", action="store_true")
    ap.add_argument("--restate-only", action="store_true", help="the host restatement on the same inputs, without the GPU runs")
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "align_time"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--tail", type=int, default=0, help="also time align --tail T on this input and on a tailed input")
    ap.add_argument("--tail-min", default="16", help="--tail-min of the timed calls; several values separated by commas")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls of each kind with --tail")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_table(a.kernel_stats), indent=1))
        return
    os.makedirs(a.dir, exist_ok=True)
    res = {"genome_bases": a.genome_mb * 1_000_000}
    gpath, rpath = os.path.join(a.dir, "genome.fa"), os.path.join(a.dir, "reads.fa")
    t = time.time()
    g = make_genome(gpath, a.genome_mb * 1_000_000, 1)
    res["reads"] = make_reads(rpath, g, a.reads, 2)
    res["reads_bytes"] = os.path.getsize(rpath)
    if a.tail:
        res["tailed_reads"] = make_reads(os.path.join(a.dir, "reads_tailed.fa"), g, a.reads, 2, tailed=True)
    res["make_inputs_s"] = time.time() - t
    if not a.restate_only:
        gpu_runs(a, gpath, rpath, res)
    if a.restate_only or not a.no_restate:
        from tests.test_align_cpu import load_reads, searchsorted_hits_v0
        t = time.time()
        rd = load_reads(rpath)
        hits = searchsorted_hits_v0([g], rd)       # one contig here: the concatenation (the timing, not the contig split, is compared)
        res["searchsorted_v0_s"] = time.time() - t
        res["searchsorted_v0_aligned"] = sum(1 for h in hits if h)
    out = a.out or os.path.join(a.dir, "align_time.json")
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))


def gpu_runs(a, gpath, rpath, res):
    from mir_prefer_amd import capi
    phases_i = ["read_parse_pack", "upload", "keys", "sort", "positions_buckets"]
    phases_r = ["read_parse", "upload", "seeds", "verify", "sort", "emit_download_write"]
    ctx = capi.Context(0)
    ctx.align_index([gpath])
    t = time.time()
    idx = ctx.align_index([gpath])
    res["index"] = {"wall_s": time.time() - t, "phases_s": dict(zip(phases_i, idx["seconds"]))}
    sam = os.path.join(a.dir, "reads.sam")
    ctx.align_reads(rpath, sam, "align_time", v=0, k=20)
    for v in ((0,) if a.tail else (0, 1, 2)):
        t = time.time()
        r = ctx.align_reads(rpath, sam, "align_time", v=v, k=20)
        res["v%d" % v] = {"wall_s": time.time() - t, "phases_s": dict(zip(phases_r, r.pop("seconds"))), **r, "sam_bytes": os.path.getsize(sam)}
        print(json.dumps({"v": v, **res["v%d" % v]}), flush=True)
    if a.tail:
        phases_t = phases_r + ["tail"]
        mins = [int(x) for x in a.tail_min.split(",")]
        res["tail"] = {"T": a.tail, "M": mins}
        for name, path in (("existing", rpath), ("tailed", os.path.join(a.dir, "reads_tailed.fa"))):
            for label, kw in [("v0", {})] + [("v0_tail_min%d" % M, {"tail": a.tail, "tail_min": M}) for M in mins]:
                ctx.align_reads(path, sam, "align_time", v=0, k=20, **kw)
                runs = []
                for _ in range(a.repeat):
                    t = time.time()
                    r = ctx.align_reads(path, sam, "align_time", v=0, k=20, **kw)
                    runs.append({"wall_s": time.time() - t, "phases_s": dict(zip(phases_t, r.pop("seconds"))), **r})
                walls = sorted(x["wall_s"] for x in runs)
                res["tail"]["%s_%s" % (name, label)] = {"wall_s_median": walls[len(walls) // 2], "wall_s_min": walls[0], "wall_s_max": walls[-1],
                                                       "last": runs[-1], "sam_bytes": os.path.getsize(sam)}
                print(json.dumps({"input": name, "call": label, **res["tail"]["%s_%s" % (name, label)]}), flush=True)
    if a.big_gb > 0:
        big = os.path.join(a.dir, "big.fa")
        make_genome(big, int(a.big_gb * 1e9), 3, n_contigs=16, repeats=False)
        t = time.time()
        idx = ctx.align_index([big])
        res["index_big"] = {"bases": idx["total"], "wall_s": time.time() - t, "phases_s": dict(zip(phases_i, idx["seconds"]))}
        os.unlink(big)
    ctx.close()


if __name__ == "__main__":
    main()

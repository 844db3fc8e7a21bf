#!/usr/bin/env python3
"""Timing of the target-mimic search (mirp_mimic_scan) on seeded inputs: about 10,000 miRNAs against a genome of about 100 Mb,
both strands, next to the brute-force target-site scan (mirp_target_scan, offsets x miRNAs) on the same files.

    python profiles/tools/mimics_time.py [--genome-mb 100] [--mirnas 10000] [--out build/mimics_time/mimics_time.json]

Genome: align_time.py's (random bases in 8 contigs, 2,000 copied segments of 1-5 kb, 200 runs of 100 N).  Two miRNA files of the same size and
lengths (20..24): `families`, in which the miRNAs of a family share positions 1..9 and family sizes are drawn from a geometric distribution (mean
4, the uneven buckets of MIR families), and `uniform`, in which every miRNA has a seed of its own draw.  Every timed call runs after a first call of
the same kind (code objects loaded).  Reports seconds[] of both scans, the seeds looked up and bucket entries evaluated, the occupancy of the seed
table, and the bytes of the packed target (2 bits per base and the two bitmaps: total / 2) over the mimic scan's seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_mirnas(path, n, families, seed):
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        head = rng.randint(0, 4, 9)
        for _ in range(int(rng.geometric(0.25)) if families else 1):
            out.append(np.concatenate([head, rng.randint(0, 4, int(rng.randint(11, 16)))]))
    out = out[:n]
    with open(path, "wb") as f:
        for i, m in enumerate(out):
            f.write(b">mir%d\n%s\n" % (i, bytes(b"ACGU"[c] for c in m)))
    keys = np.array([sum(int(c) << (2 * j) for j, c in enumerate(m[1:8])) for m in out])
    sizes = np.bincount(keys, minlength=1 << 14)
    return {"mirnas": n, "buckets_used": int((sizes > 0).sum()), "largest_bucket": int(sizes.max()),
            "mean_entries_of_a_used_bucket": float(sizes[sizes > 0].mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mb", type=int, default=100)
    ap.add_argument("--mirnas", type=int, default=10000)
    ap.add_argument("--dir", default=os.path.join(ROOT, "build", "mimics_time"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from align_time import make_genome
    from mir_prefer_amd import capi
    os.makedirs(a.dir, exist_ok=True)
    total = a.genome_mb * 1_000_000
    gpath = os.path.join(a.dir, "genome.fa")
    t = time.time()
    make_genome(gpath, total, 1)
    report = {"genome_bases": total, "make_inputs_s": None, "cases": {}}
    paths = {}
    for name in ("families", "uniform"):
        paths[name] = os.path.join(a.dir, name + ".fa")
        report["cases"][name] = {"table": make_mirnas(paths[name], a.mirnas, name == "families", 7)}
    report["make_inputs_s"] = time.time() - t
    ctx = capi.Context(0)
    out = os.path.join(a.dir, "out.tsv")
    try:
        for name in ("families", "uniform"):
            case = report["cases"][name]
            runs = [ctx.mimic_scan(paths[name], [gpath], out, both_strands=True) for _ in range(3)][1:]
            best = min(runs, key=lambda r: r["seconds"][2])
            case["mimics"] = best
            case["mimic_scan_s"] = [r["seconds"][2] for r in runs]
            case["entries_per_seed"] = best["entries"] / max(1, best["seeds"])
            case["packed_target_bytes_per_s"] = (total / 2) / best["seconds"][2]
            if name == "families":
                tg = [ctx.target_scan(paths[name], [gpath], out, both_strands=True) for _ in range(2)][1]
                case["targets_b"] = tg
                case["target_scan_s"] = tg["seconds"][2]
                case["evaluations_per_s"] = tg["evaluations"] / tg["seconds"][2]
            print(name, json.dumps(case), flush=True)
    finally:
        ctx.close()
        os.remove(out) if os.path.exists(out) else None
    text = json.dumps(report, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

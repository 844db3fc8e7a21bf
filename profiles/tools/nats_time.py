"""Times the search for natural antisense transcripts (mirp_nats_scan) on a synthetic transcriptome.

    python profiles/tools/nats_time.py [--out build/nats_time/nats_time.json] [--transcripts 35000] [--mb 70] [--planted 2000]

Input: --transcripts transcripts of uniform random letters (seeded), --mb Mb in all, as the targets of targets_time.py; --planted pairs of
transcripts share a complementary region of 100..1,500 nt with 0..10 % substitutions and, in every fourth pair, one to three indels of 1..3 nt; a
third of the transcripts end in a poly-A tail of 20..150 nt; 0.5 % of the bases lie in microsatellites of unit 1..6 and 30..300 nt.  One warm-up
call, then three, at the defaults.  Reports the seconds of every stage, the band scan's cells per second against its own vector-issue bound
(7.86e13 lane-instructions per second over the instructions per cell named in DESIGN.md §36), the numpy statement's cells per second on the band
of one found region, and how many of the planted pairs were found: a description of the seeds' sensitivity at the defaults, not a pass mark."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ISSUE_RATE = 7.86e13           # lane-instructions per second of the device
INSTRUCTIONS_PER_CELL = 11.69  # vector instructions per cell of a block of nt_scan_kernel<4, 48>, the default band
LANES_IN_USE = 48 / 64         # of a wave at the default band


def make_transcripts(n, mb, planted, seed=36):
    rng = np.random.RandomState(seed)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    mean = int(mb * 1e6) // n
    seqs = [letters[rng.randint(0, 4, int(rng.randint(mean // 4, 2 * mean - mean // 4 + 1)))] for _ in range(n)]
    budget = int(mb * 1e6) // 200
    while budget > 0:
        k = int(rng.randint(0, n))
        unit, length = letters[rng.randint(0, 4, int(rng.randint(1, 7)))], int(rng.randint(30, 301))
        if len(seqs[k]) > length:
            pos = int(rng.randint(0, len(seqs[k]) - length))
            seqs[k][pos:pos + length] = np.resize(unit, length)
        budget -= length
    pairs = []
    for _ in range(planted):
        a, b = sorted(int(x) for x in rng.choice(n, 2, replace=False))
        length = int(rng.randint(100, 1501))
        length = min(length, len(seqs[a]) - 1, len(seqs[b]) - 4)
        region = letters[rng.randint(0, 4, length)]
        copy = region.copy()
        hit = rng.random_sample(length) < rng.uniform(0, 0.10)
        copy[hit] = letters[rng.randint(0, 4, int(hit.sum()))]
        copy = list(copy)
        if rng.randint(0, 4) == 0:
            for _ in range(int(rng.randint(1, 4))):
                at, size = int(rng.randint(1, len(copy) - 4)), int(rng.randint(1, 4))
                if rng.randint(0, 2):
                    del copy[at:at + size]
                else:
                    copy[at:at] = list(letters[rng.randint(0, 4, size)])
        copy = np.array(copy[:len(seqs[b]) - 1], dtype=np.uint8)
        pa = int(rng.randint(0, len(seqs[a]) - length + 1))
        pb = int(rng.randint(0, len(seqs[b]) - len(copy) + 1))
        seqs[a][pa:pa + length] = region
        seqs[b][pb:pb + len(copy)] = comp[copy[::-1]]
        pairs.append((a, b))
    out = []
    for k, s in enumerate(seqs):
        tail = b"A" * int(rng.randint(20, 151)) if k % 3 == 0 else b""
        out.append(s.tobytes() + tail)
    return out, pairs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "nats_time", "nats_time.json"))
    ap.add_argument("--transcripts", type=int, default=35000)
    ap.add_argument("--mb", type=float, default=70)
    ap.add_argument("--planted", type=int, default=2000)
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    from mir_prefer_amd import capi
    t = time.time()
    seqs, pairs = make_transcripts(args.transcripts, args.mb, args.planted)
    result = {"transcripts": args.transcripts, "mb": args.mb, "planted": args.planted, "make_transcripts_s": round(time.time() - t, 2), "runs": []}
    bound = ISSUE_RATE / INSTRUCTIONS_PER_CELL * LANES_IN_USE
    ctx = capi.Context(0)
    recs = None
    try:
        for run in range(4):
            t = time.time()
            recs, _ = ctx.nats_scan(seqs)
            wall = time.time() - t
            st = ctx.nats_last_stats()
            rate = st["cells"] / st["seconds"][3] if st["seconds"][3] > 0 else 0.0
            entry = dict(st, wall_s=wall, warm_up=run == 0, scan_cells_per_s=rate, scan_fraction_of_issue_bound=rate / bound, records=len(recs),
                         jobs_per_slot=ctx.last_jobs_per_slot(capi.NATS_FAMILY))
            result["runs"].append(entry)
            print(json.dumps(entry), flush=True)
    finally:
        ctx.close()
    result["issue_bound_cells_per_s"] = bound
    found = {(int(r["a"]), int(r["b"])) for r in recs}
    result["planted_pairs_found"] = sum(1 for p in set(pairs) if p in found)
    result["planted_pairs"] = len(set(pairs))
    result["pairs_found_not_planted"] = len(found - set(pairs))
    if not args.skip_restatement and len(recs):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import nats_restatement as R
        r = recs[0]
        ca, cb = R.np_codes(seqs[int(r["a"])]), R.np_rc(R.np_codes(seqs[int(r["b"])]))
        t = time.time()
        got = R.np_extend(ca, cb, int(r["bin"]), 64, 3, 4, 12)
        dt = time.time() - t
        result["restatement"] = {"a_len": len(ca), "b_len": len(cb), "cells": got[6], "seconds": dt, "cells_per_s": got[6] / dt,
                                 "score_equal": got[0] == int(r["score"])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))


if __name__ == "__main__":
    main()

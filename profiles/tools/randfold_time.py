#!/usr/bin/env python3
"""Timing of the shuffle test of precursor MFEs (mirp_randfold) on seeded inputs.

    python profiles/tools/randfold_time.py [--out build/randfold_time/randfold_time.json] [--cases a,b] [--repeats 3] [--method di]

Cases (the issue's two), random sequences of 80..250 nt, seed 1:
  a  500 precursors, 999 shuffles each
  b  20,000 precursors, 99 shuffles each
Each case runs once to load the code objects and then --repeats times in the same context; the later calls are reported: median, smallest and
largest of the wall time, folds per second of the whole call, and the seconds[] split (upload, shuffle, fold, statistics, download: host clock
around each step and its synchronise).  The yardstick is what the library could do before: alternating with those calls, in the same process,
fold_batch_summary folds the very same shuffled bytes -- obtained once through shuffle_batch, every sequence followed by its shuffles, uploaded
from the host in pieces of at most --piece sequences -- with one structure line of capacity; `ratio` is the randfold wall time over that, and
`outside_fold` the share of randfold's device seconds (shuffle + fold + statistics) that is not the fold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = {"a": (500, 999), "b": (20_000, 99)}
NAMES = ("upload", "shuffle", "fold", "statistics", "download")


def make_sequences(n, seed=1):
    rng = np.random.RandomState(seed)
    acgu = np.frombuffer(b"ACGU", dtype=np.uint8)
    return [acgu[rng.randint(0, 4, size=int(L))].tobytes() for L in rng.randint(80, 251, size=n)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "randfold_time", "randfold_time.json"))
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--method", default="di", choices=["mono", "di"])
    ap.add_argument("--piece", type=int, default=1 << 18, help="sequences per fold_batch_summary call of the yardstick")
    args = ap.parse_args()
    di = args.method == "di"
    from mir_prefer_amd import capi
    ctx = capi.Context(0)
    result = {"method": args.method, "cases": {}}
    try:
        for case in args.cases.split(","):
            n, shuffles = CASES[case]
            seqs = make_sequences(n)
            t = time.time()
            rows = ctx.shuffle_batch(seqs, 0, shuffles, dinucleotide=di, seed=1)
            blob = np.frombuffer(b"".join(s + b"".join(r) for s, r in zip(seqs, rows)), dtype=np.uint8)
            offs = np.zeros(n * (shuffles + 1) + 1, dtype=np.int64)
            np.cumsum(np.repeat([len(s) for s in seqs], shuffles + 1), out=offs[1:])
            del rows
            print("case %s: %d sequences, %d letters to fold, ready in %.1f s" % (case, len(offs) - 1, len(blob), time.time() - t), flush=True)

            def yardstick():
                t = time.time()
                mfes = []
                for a in range(0, len(offs) - 1, args.piece):
                    b = min(a + args.piece, len(offs) - 1)
                    mfes.append(ctx.fold_batch_summary(blob[offs[a]:offs[b]], offs[a:b + 1] - offs[a], 300, max_lines=1)[1])
                return time.time() - t, np.concatenate(mfes)

            runs, base = [], []
            for _ in range(1 + args.repeats):
                t = time.time()
                recs, res = ctx.randfold(seqs, shuffles, dinucleotide=di, seed=1)
                res["wall_s"] = time.time() - t
                runs.append(res)
                dt, mfes = yardstick()
                base.append(dt)
            # the two agree: the records are the sums of the yardstick's MFEs
            m = mfes.reshape(n, shuffles + 1).astype(np.int64)
            assert (recs["mfe"] == m[:, 0]).all() and (recs["sum"] == m[:, 1:].sum(axis=1)).all() and (recs["le"] == (m[:, 1:] <= m[:, :1]).sum(axis=1)).all()
            later, later_base = runs[1:], base[1:]
            row = {"sequences": n, "shuffles": shuffles, "folds": runs[1]["folds"], "passes": runs[1]["passes"], "fallbacks": runs[1]["fallbacks"],
                   "first_wall_s": runs[0]["wall_s"], "wall_s": spread([r["wall_s"] for r in later]),
                   "folds_per_s": spread([r["folds"] / r["wall_s"] for r in later]),
                   "seconds": {nm: spread([r["seconds"][i] for r in later]) for i, nm in enumerate(NAMES)},
                   "fold_batch_summary_s": spread(later_base),
                   "ratio": spread([r["wall_s"] / b for r, b in zip(later, later_base)]),
                   "outside_fold": spread([(r["seconds"][1] + r["seconds"][3]) / (r["seconds"][1] + r["seconds"][2] + r["seconds"][3]) for r in later])}
            result["cases"][case] = row
            print(case, json.dumps(row), flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

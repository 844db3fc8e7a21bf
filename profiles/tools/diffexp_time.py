#!/usr/bin/env python3
"""Timing of the exact test between two groups (mirp_diffexp) on a matrix of the size of loci_time.py's.

    python profiles/tools/diffexp_time.py [--out build/diffexp_time/diffexp_time.json] [--features 375000] [--reads 29300000] [--skip-restatement]

Input: a seeded negative-binomial matrix of 375 k features x (3 + 3) samples with about 29.3 M reads in all (the clusters and reads of §31's
timing input), very uneven: eight features hold 10^6 reads each, the rest is log-normal.  One context runs mirp_diffexp twice under
`--dispersion max` and reports the second round; the numpy statement of the test (tests/diffexp_restatement.py (a)) is then timed on the same
arrays, and the run fails if a device p differs from it by more than the tolerance of tests/test_diffexp_gpu.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TOL = 64 * 1.54e-12          # tests/test_diffexp_gpu.py


def make_matrix(features, reads, seed=32):
    rs = np.random.RandomState(seed)
    heavy = 8
    mu = np.exp(rs.normal(2.2, 1.6, features))
    at = rs.choice(features, heavy, replace=False)
    mu[at] = 0.0
    phi = 0.05 + rs.uniform(0.2, 1.0, features) / np.sqrt(mu / mu.mean() * 50.0 + 1.0)
    fold = np.where(rs.uniform(size=features) < 0.1, np.exp(rs.normal(0.0, 1.0, features)), 1.0)
    depth = np.array([0.8, 1.0, 1.25, 0.9, 1.1, 1.0])
    groups = [0, 0, 0, 1, 1, 1]
    mean = mu[:, None] * depth[None, :] * np.where(np.array(groups)[None, :] == 1, fold[:, None], 1.0)
    mean *= (reads - heavy * 1_000_000) / mean.sum()
    mean[at] = 1_000_000 / 6.0 * depth[None, :]
    size = (1.0 / phi)[:, None]
    return rs.negative_binomial(size, size / (size + mean)).astype(np.uint64), groups


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "diffexp_time", "diffexp_time.json"))
    ap.add_argument("--features", type=int, default=375_000)
    ap.add_argument("--reads", type=int, default=29_300_000)
    ap.add_argument("--skip-restatement", action="store_true")
    args = ap.parse_args()
    from mir_prefer_amd import capi, diffexp
    from tests import diffexp_restatement as R
    t0 = time.time()
    counts, groups = make_matrix(args.features, args.reads)
    sf = diffexp.size_factors(counts, "mor")
    n = counts.sum(axis=1)
    print("inputs ready in %.1f s: %d features, %d reads, largest feature %d reads" % (time.time() - t0, len(counts), int(n.sum()), int(n.max())), flush=True)
    result = {"features": int(len(counts)), "samples": 6, "reads": int(n.sum()), "largest_feature": int(n.max()), "size_factors": sf.tolist()}
    ctx = capi.Context(0)
    try:
        for rnd in range(2):
            t = time.time()
            rows, stats = ctx.diffexp(counts, sf, groups, "max")
            wall = time.time() - t
            slots = ctx.last_jobs_per_slot(6)
            print("round %d: mirp_diffexp %.4f s, %s, jobs per slot %s" % (rnd, wall, stats, slots), flush=True)
        result["mirp_diffexp"] = dict(stats, wall_s=wall, jobs_per_slot=list(slots), terms_per_s=stats["terms"] / wall)
        t = time.time()
        padj = diffexp.adjust(rows["p"])
        result["adjust_s"] = time.time() - t
        result["padj_le_0.05"] = int(((padj >= 0) & (padj <= 0.05)).sum())
    finally:
        ctx.close()
    if not args.skip_restatement:
        t = time.time()
        want, phi_c = R.diffexp_numpy(counts, sf, groups, "max")
        result["numpy_restatement_s"] = time.time() - t
        with np.errstate(divide="ignore", invalid="ignore"):
            err = np.where(rows["p"] == want["p"], 0.0, np.abs(rows["p"] - want["p"]) / np.abs(want["p"]))
        result["worst_rel_difference_of_p"] = float(err.max())
        result["phi_c_restatement"] = phi_c
        print("numpy restatement %.1f s; worst relative difference of p %.3e (feature %d)" % (result["numpy_restatement_s"], err.max(), int(err.argmax())),
              flush=True)
        if not (err.max() <= TOL and phi_c == stats["phi_c"] and (rows["k_a"] == want["k_a"]).all()):
            print("the device result differs from the restatement", file=sys.stderr)
            return 1
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result["mirp_diffexp"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""The error of the float64 restatement of the exact test (tests/diffexp_restatement.py (a)) against the 60-digit one (b), on the inputs of the
GPU tests: the figure from which tests/test_diffexp_gpu.py derives its tolerance on p.  No device is used.

    python profiles/tools/diffexp_error.py [--out build/diffexp_error/diffexp_error.json] [--skip-big] [--every 10]

Runs every case of single_cases(), every `--every`-th feature of the seeded sweep under the four dispersion modes and of the 7,000 features of
the slot-reuse case and, unless --skip-big, the feature with n = 2^20 + 3 (about half a minute of mpmath).  `--every 1` takes five minutes.
Reports the worst relative error of p and the nearest any term other than k_A comes to the slack 1 + 1e-7 (the inputs must keep 1e-9 away
from it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "diffexp_error", "diffexp_error.json"))
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--every", type=int, default=10)
    args = ap.parse_args()
    from tests import diffexp_restatement as R
    worst, nearest, rows = 0.0, 1.0, []

    def one(name, n, ka, ra, rb, cr):
        nonlocal worst, nearest
        if n == 0:
            return
        t = time.time()
        got = R.p_numpy(n, ka, ra, rb, cr)
        truth, near = R.p_mp(n, ka, ra, rb, cr)
        err = 0.0 if truth < 1e-300 and got == 0.0 else float(abs(got - truth) / truth)
        rows.append({"case": name, "n": n, "k_a": ka, "p": got, "rel_err": err, "nearest_to_slack": float(near), "mpmath_s": time.time() - t})
        if err > worst:
            print("%-24s n %8d  p %.6e  rel err %.3e  nearest %.3e" % (name, n, got, err, float(near)), flush=True)
        worst, nearest = max(worst, err), min(nearest, float(near))

    for case in R.single_cases() + ([] if args.skip_big else [R.BIG]):
        one(case[0], *R.single_params(case))
    counts, sf, groups = R.sweep()
    k = R.constants(sf, groups)
    m = R.moments_numpy(counts, sf, groups)
    for mode in range(4):
        phi_c = 0.3 if mode == 3 else R.common_dispersion(m["q"], m["alpha"], 10.0)
        d = R.dispersions(m["alpha"], mode, 0.3, phi_c)
        for i in range(0, len(d), args.every):
            ka, kb = int(m["ka"][i]), int(m["kb"][i])
            one("sweep_%s_%d" % (R.MODES[mode], i), ka + kb, ka, *R.nb_params(m["q"][i], d[i], k))
    counts, sf, groups = R.sweep(seed=21, features=7000)                   # the slot-reuse case of the GPU tests, at its fixed dispersion
    k = R.constants(sf, groups)
    m = R.moments_numpy(counts, sf, groups)
    for i in range(0, len(counts), args.every):
        ka, kb = int(m["ka"][i]), int(m["kb"][i])
        one("reuse_%d" % i, ka + kb, ka, *R.nb_params(m["q"][i], 0.25, k))
    result = {"worst_rel_err": worst, "nearest_to_slack": nearest, "tolerance_64x": 64 * worst, "cases": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("worst relative error %.3e, 64 x = %.3e; nearest term to the slack %.3e; %d cases" % (worst, 64 * worst, nearest, len(rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Host tests of the accessibility of intervals (mirp_unpaired_batch, `targets -u`): §23's inside program of
tests/test_ensemble_cpu.py restated with the mask -- Qb(i,j) = 0 wherever i or j lies in the interval, nothing else changed -- which the GPU
tests (test_unpaired_gpu.py, test_targets_upe_gpu.py) compare the device with.  Here the restatement is pinned: Z_open to the enumeration of every
structure filtered by the constraint, §24's pinned values, and the identities of §24 (a single base against the pair probabilities of §23,
monotony in the interval, an interval that cannot pair).  The window of a target site as the GPU test extracts it is worked by hand, and the
command line's new option errors (exit 2 without a device) and the header's new entries are tested as well."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.test_ensemble_cpu import (KT, MAXLOOP, ML_BASE, ML_CLOSING, PAIR, RTYPE, SHORT, SumProduct, _COUNT_UP_TO, _loops, codes, e_ext, e_hairpin,
                                     e_ml, energy_of, enumerate_structures, inside, random_seq, restate, seeded)
from tests.test_targets_cpu import ROOT

HAIRPIN20 = "GGGAGCUCGAAAGAGCUCCC"
MULTI = "GGAAACGAAACC"
GC128 = "G" * 62 + "AAAA" + "C" * 62
# sequence, lo, hi (1-based) -> efe_open, efe, upe (§24, "Pins")
PINS = [(HAIRPIN20, 3, 6, -0.574530620138, -15.733592149972, 15.159061529834),
        (HAIRPIN20, 9, 12, -15.733592050972, -15.733592149972, 0.000000099000),
        (MULTI, 1, 1, -0.008353120370, -0.132199900169, 0.123846779799),
        (MULTI, 6, 7, -0.102576328390, -0.132199900169, 0.029623571779),
        ("AAAA", 1, 4, 0.0, 0.0, 0.0),
        (GC128, 1, 21, -130.603794245, -196.894162461, 66.290368217)]


def inside_open(s, lo, hi, R=SumProduct):
    """test_ensemble_cpu.inside with the mask: no position of the 1-based interval [lo, hi] pairs -> Q5[n] = Z_open"""
    S = codes(s)
    Sa = np.array(S + [0], dtype=np.int64)
    n = len(S)
    assert 1 <= lo <= hi <= n
    masked = [lo - 1 <= x <= hi - 1 for x in range(n)]
    Qb, Qm1, U, Qm, Qmm = (np.full((n + 1, n + 1), R.zero, dtype=R.dtype) for _ in range(5))
    for d in range(4, n):
        n_shapes = _COUNT_UP_TO[min(MAXLOOP, d - 6)] if d >= 6 else 0
        for i in range(n - d):
            j = i + d
            t = PAIR[S[i]][S[j]]
            if t and not masked[i] and not masked[j]:
                v = R.weight(e_hairpin(S, i, j, t))
                if d >= 6:
                    p, q, e = _loops(S, Sa, i, j, t, n_shapes)
                    keep = q - p >= 4
                    v = R.plus(v, R.total(R.times(R.weight(e[keep]), Qb[p[keep], q[keep]])))
                v = R.plus(v, R.times(R.weight(ML_CLOSING + e_ml(RTYPE[t], S[j - 1], S[i + 1])), Qmm[i + 1, j - 1]))
                Qb[i, j] = v
                Qm1[i, j] = R.plus(Qm1[i, j - 1], R.times(v, R.weight(e_ml(t, S[i - 1] if i > 0 else -1, S[j + 1] if j < n - 1 else -1))))
            else:
                Qm1[i, j] = Qm1[i, j - 1]
            assert not ML_BASE
            U[i, j] = R.plus(U[i + 1, j], Qm1[i, j])
            Qmm[i, j] = R.total(R.times(Qm[i, i + 4:j - 4], Qm1[i + 5:j - 3, j]))
            Qm[i, j] = R.plus(U[i, j], Qmm[i, j])
    Q5 = np.full(n + 1, R.one, dtype=R.dtype)
    for j in range(n):
        v = Q5[j]
        for k in range(0, j - 3):
            t = PAIR[S[k]][S[j]]
            if t:
                v = R.plus(v, R.times(R.times(Q5[k], Qb[k, j]), R.weight(e_ext(t, S[k - 1] if k > 0 else -1, S[j + 1] if j < n - 1 else -1))))
        Q5[j + 1] = v
    return Q5[n]


def restate_upe(s, lo, hi, z=None):
    """-> dict(efe, efe_open, upe) in kcal/mol; z = Z of the sequence when the caller has it"""
    z = inside(s, SumProduct)["Q5"][len(s)] if z is None else z
    zo = inside_open(s, lo, hi)
    efe, efe_open = 0.0 - KT * float(np.log(z)), 0.0 - KT * float(np.log(zo))
    return dict(efe=efe, efe_open=efe_open, upe=float(np.longdouble(KT) * (np.log(z) - np.log(zo))))


def upe_job(job):
    """(sequence, lo, hi) -> restate_upe; a module-level function so that worker processes can run it"""
    s, lo, hi = job
    return restate_upe(s.decode() if isinstance(s, bytes) else s, lo, hi)


def format_upe(upe):
    """the `upe` column of targets -u: upe x 1000 rounded to nearest, three decimals"""
    m = int(math.floor(upe * 1000 + 0.5))
    return "%d.%03d" % (m // 1000, m % 1000)


def site_window(contig, start, end, strand, up=17, down=13):
    """the window of a site (§24): contig = the forward bases of the site's contig (bytes, any case), start .. end the site's 1-based interval
    on it, strand '+' / '-' -> (window 5'->3' as ACGUN text, lo, hi of the site inside it, 1-based)"""
    before, behind = (up, down) if strand == "+" else (down, up)
    a, b = max(1, start - before), min(len(contig), end + behind)
    fwd = "".join({"A": "A", "C": "C", "G": "G", "T": "U", "U": "U"}.get(ch, "N") for ch in contig[a - 1:b].decode().upper())
    if strand == "+":
        return fwd, start - a + 1, end - a + 1
    rc = "".join({"A": "U", "C": "G", "G": "C", "U": "A"}.get(ch, "N") for ch in reversed(fwd))
    return rc, b - end + 1, b - start + 1


# ---------------------------------------------------------------------------------------------------- the restatement
def test_open_restatement_is_the_filtered_enumeration():
    rng = random.Random(2401)
    checked = constrained = 0
    for s in SHORT:
        S = codes(s)
        n = len(S)
        structs = [(pairs, energy_of(S, pairs)) for pairs in enumerate_structures(S)]
        structs = [(pairs, e) for pairs, e in structs if e is not None]
        Z = sum(np.exp(np.longdouble(-e) / np.longdouble(100 * KT)) for _, e in structs)
        for _ in range(3):
            lo = rng.randint(1, n)
            hi = rng.randint(lo, min(n, lo + rng.choice((0, 1, 3, 6))))
            keep = [e for pairs, e in structs if not any(lo - 1 <= x <= hi - 1 for ij in pairs.items() for x in ij)]
            want = sum(np.exp(np.longdouble(-e) / np.longdouble(100 * KT)) for e in keep)
            got = inside_open(s, lo, hi)
            assert abs(got - want) <= np.longdouble(1e-12) * want, (s, lo, hi)
            r = restate_upe(s, lo, hi)
            assert abs(r["upe"] - float(np.longdouble(KT) * (np.log(Z) - np.log(want)))) <= 1e-12, (s, lo, hi)
            checked += 1
            constrained += len(keep) < len(structs)
    assert checked == 3 * len(SHORT) and constrained > 60


def test_pins():
    for s, lo, hi, efe_open, efe, upe in PINS:
        r = restate_upe(s, lo, hi)
        assert abs(r["efe_open"] - efe_open) <= 2e-9 and abs(r["efe"] - efe) <= 2e-9 and abs(r["upe"] - upe) <= 2e-9, (s, lo, hi, r)
    r = restate_upe("AAAA", 1, 4)
    assert r["efe"] == 0.0 and r["efe_open"] == 0.0 and r["upe"] == 0.0


def test_single_base_is_the_unpaired_probability():
    worst = 0.0
    for s in seeded(2402, 12, 30, 70):
        r = restate(s)
        n = r["n"]
        rows = [0.0] * n
        for (i, j), v in r["p"].items():
            rows[i] += v
            rows[j] += v
        z = inside(s, SumProduct)["Q5"][n]
        for a in random.Random(len(s)).sample(range(n), 3):
            got = restate_upe(s, a + 1, a + 1, z)["upe"]
            want = 0.0 - KT * math.log(1.0 - rows[a])
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-9, (s, a)
    print("single base: largest difference %.3g kcal/mol" % worst)


def test_monotony_and_an_interval_that_cannot_pair():
    rng = random.Random(2403)
    for s in seeded(2404, 6, 24, 48):
        n = len(s)
        z = inside(s, SumProduct)["Q5"][n]
        lo = rng.randint(3, n - 6)
        hi = lo + rng.randint(0, 3)
        inner = restate_upe(s, lo, hi, z)["upe"]
        assert inner >= 0
        for lo2, hi2 in ((lo - 2, hi), (lo, hi + 2), (1, n)):
            assert restate_upe(s, lo2, hi2, z)["upe"] >= inner - 1e-12, (s, lo, hi, lo2, hi2)
    assert restate_upe("A" * 40, 7, 19)["upe"] == 0.0
    s = "GGGGC" + "A" * 9 + "GCCCC"          # the run of A pairs with nothing here: opening it costs nothing
    assert restate_upe(s, 6, 14)["upe"] == 0.0 and restate_upe(s, 2, 3)["upe"] > 1.0


# ---------------------------------------------------------------------------------------------------- the window of a site
def test_site_window_by_hand():
    contig = b"acgtnACGTTGCAAGGCTTAAGGCCTTAGCAT"          # 32 bases; [10, 14] = TGCAA
    # plus strand, inside the contig: 3 up = [7, 9] = CGT, 2 down = [15, 16] = GG
    assert site_window(contig, 10, 14, "+", 3, 2) == ("CGUUGCAAGG", 4, 8)
    # plus strand, clipped at the contig's start (one base before the site) and at its end (two behind it)
    assert site_window(contig, 2, 4, "+", 17, 2) == ("ACGUNA", 2, 4)
    assert site_window(contig, 27, 30, "+", 1, 13) == ("UUAGCAU", 2, 5)
    # minus strand: the reverse complement of [start - down, end + up] = [8, 17] = GTTGCAAGGC; the site counted from the window's 5' end
    w, lo, hi = site_window(contig, 10, 14, "-", 3, 2)
    assert (w, lo, hi) == ("GCCUUGCAAC", 4, 8) and w[lo - 1:hi] == "UUGCA"
    # minus strand, clipped: `down` is cut at the contig's start ([1, 5] = acgtn), `up` at its end ([29, 32] = GCAT)
    assert site_window(contig, 2, 4, "-", 1, 13) == ("NACGU", 2, 4)
    assert site_window(contig, 29, 31, "-", 17, 0) == ("AUGC", 2, 4)
    # a contig shorter than a window, an ambiguous base as N; no flanks
    assert site_window(b"ACGTRACG", 2, 7, "+") == ("ACGUNACG", 2, 7) and site_window(b"ACGTRACG", 2, 7, "-") == ("CGUNACGU", 2, 7)
    assert site_window(contig, 10, 14, "+", 0, 0) == ("UGCAA", 1, 5)
    assert [format_upe(x) for x in (0.0, 15.159061529834, 0.0004, 0.0006, 9.9996)] == ["0.000", "15.159", "0.000", "0.001", "10.000"]


# ---------------------------------------------------------------------------------------------------- the command line and the header
def test_option_errors_exit_2_before_a_device(tmp_path):
    mir, tgt = tmp_path / "m.fa", tmp_path / "t.fa"
    mir.write_bytes(b">m\nUUCCACAGCUUUCUUGAACUG\n")
    tgt.write_bytes(b">t\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    bad = [["--flank-up", "5"], ["--flank-down", "5"], ["-u", "--flank-up", "-1"], ["-u", "--flank-down", "-1"], ["-u", "--flank-up", "90", "--flank-down", "6"],
           ["-u", "--flank-up", "x"], ["-u", "--flank-up", "96"]]
    for extra in bad:
        r = subprocess.run([sys.executable, "-m", "mir_prefer_amd.targets"] + extra + [str(mir), str(tgt)], cwd=str(tmp_path), capture_output=True, timeout=120,
                           env=dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2 and b"Error: " not in r.stderr, (extra, r.stderr.decode())
    assert not [p for p in tmp_path.iterdir() if p.name not in ("m.fa", "t.fa")]


def test_abi_entries_are_declared():
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    for name in ("mirp_unpaired_batch(", "mirp_set_unpaired_capacity(", "mirp_unpaired_last_stats(", "mirp_set_target_flanks(", "MirpUnpairedRec",
                 "int32_t energy, accessibility;"):
        assert name in header, name
    assert "#define MIRP_ABI_VERSION 17 " in open(os.path.join(ROOT, "mir-prefer_amd", "csrc", "mirp_api.cpp")).read()          # only entries are added
    from mir_prefer_amd import capi
    assert capi.UNPAIRED_DTYPE.itemsize == 24 and capi.UNPAIRED_DTYPE.names == ("efe", "efe_open", "upe")
    import ctypes
    assert ctypes.sizeof(capi.TargetOpts) == 32 and capi.TargetOpts.accessibility.offset == 28

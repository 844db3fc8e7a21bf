"""GPU tests of the inverted-repeat search (mirp_inverted_scan, mir_prefer_amd.inverted).  Every comparison is exact equality with
the restatement of tests/inverted_restatement.py: records, structures, the counts of rows, candidates and accepted repeats, and the bytes of the
three files.

The row scan's tile (8,192 rows) is longer than the largest span (4,096), so the two arms of a repeat lie in the same tile or in adjacent ones;
"the left arm in one unit, the right arm in the next and in the one after" is tested on the strips (1,024 rows), the unit between which the
kernel hands H on, and on tiles as far as a span reaches.  A wave serves one tile, so there is no family of mirp_last_jobs_per_slot to test."""
import os
import random
import subprocess
import sys

import pytest

from tests import inverted_restatement as R
from tests.test_targets_cpu import ROOT

pytestmark = pytest.mark.gpu

T, STRIP = 8192, 1024
S6 = dict(min_score=6, max_span=8)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def plant(genome, rng, pos, arm, loop, subs=0, deleted=False):
    """writes a repeat with its left arm at 0-based pos into the list of letters `genome`: arm + loop + arm bases (one fewer with `deleted`)"""
    left = [rng.choice("ACGT") for _ in range(arm)]
    right = list(revcomp("".join(left)))
    for _ in range(subs):
        p = rng.randrange(3, arm - 3)
        right[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[right[p]]
    if deleted:
        del right[arm // 2]
    genome[pos:pos + arm] = left
    genome[pos + arm + loop:pos + arm + loop + len(right)] = right


def as_tuples(recs):
    return [(r["contig"], r["score"], r["left_start"], r["left_end"], r["right_start"], r["right_end"], r["matches"], r["mismatches"], r["gaps"], 0)
            for r in recs]


def n_cells(contigs, max_span):
    return sum(min(max_span - 1, len(c) - i) for c in contigs for i in range(1, len(c) + 1))


def run(ctx, contigs, capacity=0, **opts):
    o = dict(R.DEFAULTS, **opts)
    recs, structures = ctx.inverted_scan(contigs, capacity=capacity, **o)
    return [tuple(r) for r in recs.tolist()], structures, ctx.inverted_last_stats()


def check(ctx, contigs, capacity=0, want=None, **opts):
    o = dict(R.DEFAULTS, **opts)
    if want is None:
        st = {}
        want = (R.find(contigs, stats=st, **o), st)
    exp, st = want
    recs, structures, stats = run(ctx, contigs, capacity, **o)
    assert len(recs) == len(exp)
    for got, gs, e, es in zip(recs, structures, as_tuples(exp), [R.structure(r["ops"]) for r in exp]):
        assert got == e and gs == es, (got, gs, e, es)
    assert (stats["rows_above"], stats["candidates"], stats["accepted"]) == (st["rows_above"], st["candidates"], st["accepted"])
    assert stats["traced"] + stats["dropped_untraced"] == stats["candidates"] and stats["traced"] >= stats["accepted"]
    assert (stats["contigs"], stats["bases"]) == (len(contigs), sum(len(c) for c in contigs))
    assert stats["cells"] == n_cells(contigs, o["max_span"])
    return recs, structures, stats, want


def test_pins_on_the_device(gpu_ctx):
    recs, structures, _ = run(gpu_ctx, ["ACGT"], **S6)
    assert recs == [(0, 6, 1, 2, 3, 4, 2, 0, 0, 0)] and structures == ["2="]
    # 9 nt: within a span of 9 the whole of it, within 8 its inner part, as the recurrence gives it
    assert run(gpu_ctx, ["GGGAAACCC"], min_score=6, max_span=9)[:2] == ([(0, 9, 1, 3, 7, 9, 3, 0, 0, 0)], ["3="])
    assert run(gpu_ctx, ["GGGAAACCC"], **S6)[:2] == ([(0, 6, 1, 2, 7, 8, 2, 0, 0, 0)], ["2="])
    assert run(gpu_ctx, ["GGGNCCC"], **S6)[:2] == ([(0, 9, 1, 3, 5, 7, 3, 0, 0, 0)], ["3="])
    assert run(gpu_ctx, [], **S6)[0] == [] and run(gpu_ctx, ["", "A", ""], **S6)[0] == []
    assert run(gpu_ctx, ["ACGT"], min_score=7, max_span=8)[0] == []


@pytest.mark.parametrize("alphabet", ["AT", "ACGT"])
@pytest.mark.parametrize("D", [8, 63, 64, 65, 257])
def test_lengths_around_the_span_and_the_tile(gpu_ctx, D, alphabet):
    rng = random.Random(1000 * D + len(alphabet))
    contigs = [rand_seq(rng, n, alphabet) for n in (1, 2, 3, D - 1, D, D + 1, T - 1, T, T + 1, 2 * T + 1)]
    recs, _, stats, _ = check(gpu_ctx, contigs, min_score=6, max_span=D)
    assert len(recs) > 100 and {r[0] for r in recs} >= {6, 7, 8, 9}
    assert stats["tiles"] >= 5 and stats["scan_passes"] == 1


def test_many_short_contigs(gpu_ctx):
    rng = random.Random(5)
    contigs = [rand_seq(rng, rng.randint(1, 40), "AT" if k % 3 else "ACGT") for k in range(100)]
    recs, _, _, _ = check(gpu_ctx, contigs, min_score=6, max_span=30)
    assert len({r[0] for r in recs}) > 40


def test_no_record_crosses_contigs(gpu_ctx):
    rng = random.Random(6)
    first = rand_seq(rng, 200)
    pair = [first, revcomp(first)]
    recs, _, _, _ = check(gpu_ctx, pair, min_score=20, max_span=500)
    alone = [check(gpu_ctx, [c], min_score=20, max_span=500)[0] for c in pair]
    assert recs == alone[0] + [(1,) + r[1:] for r in alone[1]]
    whole = run(gpu_ctx, [first + revcomp(first)], min_score=20, max_span=500)[0]          # as one contig it is one long repeat
    assert max(r[1] for r in whole) == 3 * 200 and max([r[1] for r in recs] or [0]) < 100


def test_planted_repeats_at_the_boundaries(gpu_ctx):
    rng = random.Random(7)
    D = 2500
    g = [rng.choice("ACGT") for _ in range(3 * T + 100)]
    spots = [(STRIP - 50, 40, 30),               # left arm in one strip, right arm in the next
             (3 * STRIP - 45, 40, 1100),         # ... and in the one after
             (T - 60, 50, 100),                  # left arm in one tile, right arm in the next
             (2 * T - 30, 60, 2300),             # across a tile's end at nearly the whole span
             (T + 5 * STRIP - 1, 30, 10),        # starts on a strip's last row
             (T - 1, 30, 500),                   # starts on a tile's last row
             (3 * T + 100 - 70, 30, 10)]         # ends with the contig
    for pos, arm, loop in spots:
        plant(g, rng, pos, arm, loop, subs=1 if arm >= 40 else 0)
    recs, _, _, _ = check(gpu_ctx, ["".join(g)], max_span=D)
    for pos, arm, loop in spots:
        # (the background may pair a base or two beyond either end, and a substitution near an end may cost a base or two)
        assert any(abs(r[2] - (pos + 1)) <= 3 and abs(r[5] - (pos + 2 * arm + loop)) <= 3 and r[1] >= 3 * arm - 16 for r in recs), (pos, arm, loop)
    # a repeat within the last D rows of a contig that is followed by another contig
    check(gpu_ctx, ["".join(g[:T + 300]), "".join(g[T - 200:2 * T])], max_span=D)


@pytest.mark.parametrize("extra", [0, 1, 2])
def test_extent_at_and_past_the_span(gpu_ctx, extra):
    rng = random.Random(8)
    D, arm = 300, 40
    g = [rng.choice("AC") for _ in range(1000)]          # (no pair in the background)
    plant(g, rng, 350, arm, D + extra - 2 * arm)
    recs, structures, _, _ = check(gpu_ctx, ["".join(g)], max_span=D)
    shorter = (extra + 1) // 2                                # pairs whose cell lies outside the band
    assert recs == [(0, 3 * (arm - shorter), 351 + shorter, 350 + arm, 351 + D + extra - arm, 350 + D + extra - shorter, arm - shorter, 0, 0, 0)]
    assert structures == ["%d=" % (arm - shorter)]


def test_letters(gpu_ctx):
    rng = random.Random(9)
    base = rand_seq(rng, 600)
    variants = [base.lower(), base.replace("T", "U"), base.replace("T", "u"), "".join(c if rng.random() > 0.05 else rng.choice("NnRY-*x.") for c in base)]
    want = None
    for v in variants[:3]:
        want = check(gpu_ctx, [v], want=want, min_score=12, max_span=100)[3]
        assert check(gpu_ctx, [base], want=want, min_score=12, max_span=100)[0]
    recs, _, _, _ = check(gpu_ctx, [variants[3]], min_score=12, max_span=100)
    assert recs and recs != check(gpu_ctx, [base], min_score=12, max_span=100)[0]
    from mir_prefer_amd import capi
    with pytest.raises(capi.MirpError, match=r"\(-10\).*contig 2: a byte >= 0x80"):
        gpu_ctx.inverted_scan([b"ACGT", b"AC\x80T", b"\xff"], **S6)
    assert gpu_ctx.inverted_last_stats()["contigs"] == 0
    for bad in (dict(max_span=7), dict(max_span=4097), dict(min_score=0), dict(match=11), dict(mismatch=0), dict(gap=51)):
        with pytest.raises(capi.MirpError, match=r"\(-1\)"):
            gpu_ctx.inverted_scan(["ACGT"], **dict(S6, **bad))


def test_homopolymers_and_microsatellites(gpu_ctx):
    assert run(gpu_ctx, ["A" * 500, "c" * 500], min_score=3, max_span=64)[0] == []
    recs, structures, _, _ = check(gpu_ctx, ["AT" * 60], max_span=400)
    assert [r[1:6] for r in recs] == [(180, 1, 60, 61, 120)] and structures == ["60="]
    rng = random.Random(10)
    units = ["AT", "TA", "CG", "AAT", "ACGT", "GAATTC", "AG", "ATT"]
    contigs = [rand_seq(rng, 50) + u * (300 // len(u)) + rand_seq(rng, 50) for u in units]
    check(gpu_ctx, contigs + ["AT" * 1500], max_span=257, min_score=20)


def test_whole_span_palindrome(gpu_ctx):
    rng = random.Random(11)
    left = rand_seq(rng, 2048)
    recs, structures, stats = run(gpu_ctx, [left + revcomp(left)], max_span=4096, match=10, min_score=20000)
    assert recs == [(0, 20480, 1, 2048, 2049, 4096, 2048, 0, 0, 0)] and structures == ["2048="]
    assert stats["cells"] == 4096 * 4095 // 2


def test_noisy_repeat_of_the_whole_span(gpu_ctx):
    rng = random.Random(12)
    g = [rng.choice("ACGT") for _ in range(4700)]
    plant(g, rng, 300, 1900, 295, subs=150, deleted=True)          # extent 4,094
    for k in range(12):                                              # ... and single bases taken out of the left arm
        del g[400 + 120 * k]
    recs, structures, _, _ = check(gpu_ctx, ["".join(g)], max_span=4096, match=10, mismatch=10, gap=50, min_score=2000)
    assert recs[0][1] > 10000 and recs[0][5] - recs[0][2] + 1 == 4096 and recs[0][8] >= 10 and "R" in structures[0] and "X" in structures[0]


def test_splits_give_the_same_records(gpu_ctx):
    rng = random.Random(13)
    g = [rng.choice("ACGT") for _ in range(2 * T + 500)]
    for k in range(12):
        plant(g, rng, 700 + 1300 * k, 30 + 5 * k, 20 * k, subs=k % 3)
    contigs = ["".join(g), rand_seq(rng, 700, "AT")]
    recs, structures, stats, want = check(gpu_ctx, contigs, min_score=24, max_span=300)
    assert stats["scan_passes"] == 1 and stats["trace_passes"] == 1 and stats["traced"] > 50
    got = check(gpu_ctx, contigs, capacity=1, want=want, min_score=24, max_span=300)
    assert got[:2] == (recs, structures)
    assert got[2]["scan_passes"] == got[2]["tiles"] == 3 and got[2]["trace_passes"] == got[2]["traced"]
    assert got[2]["dropped_untraced"] >= stats["dropped_untraced"]
    mid = check(gpu_ctx, contigs, capacity=4 * T + 40000, want=want, min_score=24, max_span=300)[2]
    assert mid["scan_passes"] == 2 and 1 < mid["trace_passes"] < mid["traced"]


def test_alone_together_and_shuffled(gpu_ctx):
    rng = random.Random(14)
    contigs = [rand_seq(rng, n, a) for n, a in ((900, "ACGT"), (1025, "AT"), (17, "AT"), (T + 3, "ACGT"), (300, "AT"), (1, "A"), (2048, "ACGT"))]
    o = dict(min_score=15, max_span=120)
    alone = [check(gpu_ctx, [c], **o)[:2] for c in contigs]
    together = check(gpu_ctx, contigs, **o)[:2]
    assert together[0] == [(k,) + r[1:] for k, (recs, _) in enumerate(alone) for r in recs]
    assert together[1] == [s for _, structures in alone for s in structures]
    order = list(range(len(contigs)))
    rng.shuffle(order)
    shuffled = run(gpu_ctx, [contigs[k] for k in order], **o)[:2]
    assert shuffled[0] == [(pos,) + r[1:] for pos, k in enumerate(order) for r in alone[k][0]]
    assert shuffled[1] == [s for k in order for s in alone[k][1]]


def test_command_line(tmp_path):
    from mir_prefer_amd import gffmask
    rng = random.Random(15)
    g = [rng.choice("ACGT") for _ in range(3000)]
    for pos, arm, loop, subs in ((100, 25, 0, 0), (600, 60, 40, 2), (1500, 90, 150, 3), (2300, 40, 100, 1)):
        plant(g, rng, pos, arm, loop, subs)
    contigs = ["".join(g).lower(), "AT" * 60, "ACGTNNNNACGU"]
    names = ["chr1", "sat|2", "tiny"]
    fa = tmp_path / "genome.fa"
    fa.write_text("".join(">%s some words\n%s\n" % (n, "\n".join(c[i:i + 70] for i in range(0, len(c), 70))) for n, c in zip(names, contigs)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "mir_prefer_amd.inverted"]
    p = subprocess.run(cmd + ["-d", "400", str(fa)], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    exp = R.find(contigs, max_span=400)
    assert len(exp) == 5
    base = str(fa) + ".inverted"
    assert open(base + ".tsv").read() == R.tsv_text(names, exp)
    assert open(base + ".gff3").read() == R.gff_text(names, exp)
    assert open(base + ".fa").read() == R.fasta_text(names, contigs, exp)
    assert "3 contigs, 3132 bases" in p.stderr and "5 accepted" in p.stderr and p.stderr.count("\n") == 1
    regions = gffmask.keep_regions_include(base + ".gff3")
    assert sorted(regions) == sorted((names[r["contig"]], r["left_start"] - 1, r["right_end"]) for r in exp if r["right_end"] - r["left_start"] >= 55)
    # -o, no repeat: headers only, no error
    other = str(tmp_path / "out" )
    p = subprocess.run(cmd + ["-s", "5000", "-o", other, str(fa)], env=env, capture_output=True, text=True)
    assert p.returncode == 0 and open(other + ".tsv").read() == R.TSV_HEADER and open(other + ".gff3").read() == "##gff-version 3\n"
    assert open(other + ".fa").read() == "" and "0 accepted" in p.stderr
    # a refused input and a missing one exit with 255 and leave no file, not even the earlier run's; an option error exits with 2
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">x\nACGT\n>y\nAC\xe9T\n")
    p = subprocess.run(cmd + ["-o", other, str(fa), str(bad)], env=env, capture_output=True, text=True)
    assert p.returncode == 255 and p.stderr.startswith("Error: ") and "contig 5" in p.stderr
    assert not any(os.path.exists(other + ext) for ext in (".tsv", ".gff3", ".fa"))
    twice = tmp_path / "twice.fa"
    twice.write_text(">a\nACGT\n>a\nACGT\n")
    p = subprocess.run(cmd + [str(twice)], env=env, capture_output=True, text=True)
    assert p.returncode == 255 and "occurs twice" in p.stderr and not os.path.exists(str(twice) + ".inverted.tsv")
    p = subprocess.run(cmd + [str(tmp_path / "missing.fa")], env=env, capture_output=True, text=True)
    assert p.returncode == 255 and p.stderr.startswith("Error: ")
    p = subprocess.run(cmd + ["-d", "5000", str(fa)], env=env, capture_output=True, text=True)
    assert p.returncode == 2

"""CPU tests of the miRNA triggers of PHAS loci (mir_prefer_amd.triggers): the two restatements of tests/trigger_restatement.py
agree on the seeded inputs the GPU tests use; the hand-worked examples of §29; the phas.tsv reader; and the option errors and file refusals of the
command line, which happen before a device is opened."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd import phasing, triggers
from tests.test_phasing_cpu import ROOT, make_records
from tests.test_targets_cpu import _mutate, parse_mirnas, target_of_mirna
from tests.trigger_restatement import HEADER, SUMMARY_HEADER, cut_and_register, restate_numpy, restate_plain, window_start

GRID = [(10, Fraction(1, 1000), 3, 1), (4, Fraction(1, 100), 2, 2), (20, Fraction(1, 10 ** 5), 5, 1), (7, Fraction(1), 1, 3)]   # test_phasing_gpu.GRID
NAMES, LENS = ["chrB", "short", "chrA", "chrC"], [3000, 150, 5000, 900]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- seeded inputs (also used on the GPU)
def _mirna(rng, L, fixed=()):
    s = bytearray(b"ACGU"[c] for c in rng.randint(0, 4, L))
    for i, ch in fixed:
        s[i - 1] = ord(ch)
    return bytes(s)


def make_case(seed, Lp, m, flank):
    """A genome of four contigs, miRNAs, records and loci with every plant of the GPU grid.  -> dict(seqs, mirnas (FASTA bytes), alns, rows, plants);
    plants[name] = (locus index, miRNA name) of the plant.  The planted registers depend on Lp and m; the edge plant on flank."""
    rng = np.random.RandomState(seed)
    seqs = [bytearray(ACGT[rng.randint(0, 4, ln)].tobytes()) for ln in LENS]
    mirs = {"m21": _mirna(rng, 21), "m22": _mirna(rng, 22), "m12": _mirna(rng, 12), "m32": _mirna(rng, 32), "mm10": _mirna(rng, 21, [(10, "A")]),
            "gu11": _mirna(rng, 21, [(11, "G")]), "nin": _mirna(rng, 21), "edge": _mirna(rng, 21), "shared": _mirna(rng, 20), "rnd1": _mirna(rng, 24),
            "rnd2": _mirna(rng, 19)}
    cyc = min(8, m)
    rows, recs, plants = [], [], {}

    def reads(tid, strand, side, x):
        """Phased reads on both strands in the cyc cycles next to the cut of the window at register x; -> their coordinates."""
        js = range(cyc) if (strand == 0) == (side == 0) else range(m - cyc, m)
        cs = [x + j * Lp for j in js if x + j * Lp >= 3]
        for c in cs:
            recs.append((tid, c, int(rng.randint(3, 31)), Lp, 0))
            recs.append((tid, c - 2, int(rng.randint(3, 31)), Lp, 1))
        return cs

    def plant(name, mir, tid, o, strand, side, delta, site=None, row=True, off_register=0):
        L = len(mirs[mir])
        seqs[tid][o:o + L] = site if site is not None else target_of_mirna(mirs[mir].replace(b"U", b"T"), strand)
        _, r = cut_and_register(o, L, strand, Lp)
        x = window_start(r, strand, side, delta, m, Lp)
        cs = reads(tid, strand, side, x)
        if row:
            lo, hi = max(1, min(o + 1, cs[0])), min(LENS[tid], max(o + L, cs[-1] + Lp - 1))
            plants[name] = (len(rows), mir.encode())
            rows.append((NAMES[tid], lo, hi, cs[0] + off_register))
        return r, cs

    A, B, C = 2, 0, 3
    plant("plus_down", "m21", A, 500, 0, 0, 0)
    plant("minus_down", "m21", A, 1100, 1, 0, 0, off_register=1)
    plant("plus_up", "m22", A, 1700, 0, 1, 0)
    plant("minus_up", "m22", A, 2300, 1, 1, 0, off_register=1)
    plant("drift_p1", "m21", A, 2900, 0, 0, 1)
    plant("drift_m2", "m22", A, 3500, 1, 0, -2)
    plant("len12", "m12", A, 4100, 0, 0, 0)
    plant("drift_m1", "m22", A, 4600, 0, 1, -1)
    plant("len32", "m32", B, 400, 1, 1, 0)
    L = 21
    plant("mismatch10", "mm10", B, 1000, 0, 0, 0, site=_mutate(target_of_mirna(mirs["mm10"].replace(b"U", b"T")), L, 10, "C"))
    plant("gu11", "gu11", B, 1600, 0, 0, 0, site=_mutate(target_of_mirna(mirs["gu11"].replace(b"U", b"T")), L, 11, "T"))
    nsite = bytearray(target_of_mirna(mirs["nin"].replace(b"U", b"T")))
    nsite[5] = ord("N")
    plant("n_inside", "nin", B, 2200, 0, 0, 0, site=bytes(nsite))
    plant("drift_p2", "m21", B, 2600, 1, 1, 2)
    plant("contig_end", "m21", B, LENS[B] - 21, 1, 0, 0)                          # the site's last base is the contig's last
    assert rows[-1][2] == LENS[B]
    # the contig start: the plus site's `up` window starts below coordinate 1; its `down` window is planted
    r, _ = plant("contig_start", "m22", C, 20, 0, 0, 0)
    reads(C, 0, 1, window_start(r, 0, 1, 0, m, Lp))
    assert window_start(r, 0, 1, 0, m, Lp) <= 0
    rows[-1] = (NAMES[C], 1, rows[-1][2], rows[-1][3])
    # a plus site past the end of its locus, `up`: its last base is one past the interval's edge at this flank
    o = 600
    r, cs = plant("edge", "edge", C, o, 0, 1, 0, row=False)
    end = o + 21 - flank - 1
    plants["edge"] = (len(rows), b"edge")
    rows.append((NAMES[C], min(cs[0], end - 40), end, cs[0]))
    # two loci whose flanks share one site: one holds the siRNAs, the other ends 5 nt before the site
    r, cs = plant("shared_a", "shared", C, 300, 0, 0, 0)
    plants["shared_b"] = (len(rows), b"shared")
    rows.append((NAMES[C], 300 - 60, 300 - 5, cs[0]))
    # a locus with reads and no site, on the contig shorter than a window
    plants["no_site"] = (len(rows), None)
    for c in range(20, 20 + 4 * Lp, Lp):
        recs.append((1, c, 5, Lp, 0))
        recs.append((1, c - 2, 4, Lp, 1))
    rows.append((NAMES[1], 20, 120, 20))
    for _ in range(400):                                                         # noise of mixed lengths
        tid = int(rng.randint(0, 4))
        ln = int((18, 20, 21, 22, 23, 24, 26)[rng.randint(0, 7)])
        recs.append((tid, int(rng.randint(1, LENS[tid] - ln + 2)), int(rng.randint(1, 20)), ln, int(rng.randint(0, 2))))
    fasta = b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in mirs.items())
    return dict(seqs=[bytes(s) for s in seqs], mirna_fasta=fasta, mirnas=parse_mirnas(fasta), alns=make_records(recs), rows=rows, plants=plants)


def grid_cases():
    """(Lp, m, alpha, K, D, flank, drift) of the GPU grid: Lp 21 / 22 / 24 x the four settings, drift and flank cycling; the first is the default."""
    out = []
    for i, Lp in enumerate((21, 22, 24)):
        for j, (m, alpha, K, D) in enumerate(GRID):
            out.append((Lp, m, alpha, K, D, (100, 30, 0, 57)[j], (0, 1, 2)[(i + j) % 3]))
    return out


def lines_of(tsv):
    return [ln.split(b"\t") for ln in tsv.split(b"\n")[1:-1]]


def check_plants(case, tsv, summ, flank, drift, K):
    """What the plants guarantee in the files of one grid case (the setting (7, 1, 1, 3) passes every window with a phased unit)."""
    rows = lines_of(tsv)
    loci = ["%s:%d-%d" % r[:3] for r in case["rows"]]

    def has(name, strand=None, side=None, offset=None):
        q, mir = case["plants"][name]
        return any(r[0] == loci[q].encode() and r[1] == mir and (strand is None or r[5] == strand) and (side is None or r[11] == side) and
                   (offset is None or r[12] == offset) for r in rows)
    kinds = {(r[5], r[11]) for r in rows}
    assert kinds == {(b"+", b"down"), (b"+", b"up"), (b"-", b"down"), (b"-", b"up")}
    assert has("plus_down", b"+", b"down", b"0") and has("minus_down", b"-", b"down", b"0") and has("plus_up", b"+", b"up", b"0")
    assert has("minus_up", b"-", b"up", b"0") and has("len12", b"+", b"down", b"0") and has("len32", b"-", b"up", b"0")
    assert has("gu11", b"+", b"down", b"0") and has("contig_end", b"-", b"down", b"0") and has("contig_start", b"+", b"down", b"0")
    assert not has("mismatch10") and not has("n_inside") and not has("edge")
    for name, strand, side, delta in (("drift_p1", b"+", b"down", 1), ("drift_m2", b"-", b"down", -2), ("drift_m1", b"+", b"up", -1),
                                      ("drift_p2", b"-", b"up", 2)):
        assert has(name, strand, side, b"%d" % delta) == (abs(delta) <= drift), (name, drift)
        if K > 1:                                           # off the register no window of the plant has K phased units
            assert has(name) == (abs(delta) <= drift), (name, drift)
    if flank >= 25:
        assert has("shared_a", b"+", b"down", b"0") and has("shared_b", b"+", b"down", b"0")
    s = lines_of(summ)
    assert len(s) == len(case["rows"]) and s[case["plants"]["no_site"][0]][1:] == [b"0", b"0", b".", b".", b".", b"."]
    assert s[case["plants"]["plus_down"][0]][3:6] == [b"m21", b"down", b"0"]
    return len(rows)


# ---------------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("case_id", range(12))
def test_numpy_restatement_agrees_with_the_plain_one(case_id):
    Lp, m, alpha, K, D, flank, drift = grid_cases()[case_id]
    case = make_case(100 + case_id, Lp, m, flank)
    kw = dict(Lp=Lp, m=m, alpha=alpha, K=K, D=D, flank=flank, drift=drift)
    tsv, summ = restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    assert (tsv, summ) == restate_plain(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    assert check_plants(case, tsv, summ, flank, drift, K) >= 9
    # the edge plant: one base more of flank takes its site in
    kw["flank"] = flank + 1
    tsv1, _ = restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    q, mir = case["plants"]["edge"]
    edge = [r for r in lines_of(tsv1) if r[1] == mir]
    assert edge and all(r[5] == b"+" and r[11] == b"up" for r in edge if r[12] == b"0")


# ---------------------------------------------------------------------------------------------------- the hand-worked examples of §29
def _hand(strand, side):
    """A seeded 3 kb contig, a 22-nt miRNA whose site has one mismatch at position 18, 21-nt reads on both strands at the 8 cycles next to the cut."""
    rng = np.random.RandomState(29)
    seq = bytearray(ACGT[rng.randint(0, 4, 3000)].tobytes())
    mir = b"UGGACUGAAGGGAGCUCCUUCU"
    assert len(mir) == 22
    site = bytearray(target_of_mirna(mir.replace(b"U", b"T"), strand))
    j = 22 - 18 if strand == 0 else 18 - 1                   # the forward base paired with miRNA position 18 (C): G -> T on +, C -> A on -
    assert site[j:j + 1] == (b"G" if strand == 0 else b"C")
    site[j] = ord("T" if strand == 0 else "A")
    o, Lp, m = 1500, 21, 10
    seq[o:o + 22] = site
    cut, r = cut_and_register(o, 22, strand, Lp)
    x = window_start(r, strand, side, 0, m, Lp)
    js = range(8) if (strand == 0) == (side == 0) else range(2, 10)
    recs = []
    for jj in js:
        recs += [(0, x + jj * Lp, 5, 21, 0), (0, x + jj * Lp - 2, 3, 21, 1)]
    lo = min(o + 1, x + js[0] * Lp)
    hi = max(o + 22, x + js[-1] * Lp + 20)
    rows = [("c", lo, hi, x + js[0] * Lp)]
    mirnas = parse_mirnas(b">miR-hand\n" + mir + b"\n")
    out = restate_plain(make_records(recs), ["c"], [bytes(seq)], mirnas, rows, flank=0)
    assert out == restate_numpy(make_records(recs), ["c"], [bytes(seq)], mirnas, rows, flank=0)
    return lines_of(out[0]), lines_of(out[1]), o, cut, r, rows[0]


def _p16():
    S, G = 420, 20
    return b"%.3e" % float(Fraction(math.comb(G, 16) * math.comb(S - G, 0), math.comb(S, 16)))


def test_hand_example_plus_down():
    rows, summ, o, cut, r, locus = _hand(0, 0)
    assert len(rows) == 1
    f = rows[0]
    assert cut == o + 22 - 9 == 1513 and r == cut                  # §18's p: the target base paired with miRNA position 10, 1-based
    assert f[:13] == [b"c:%d-%d" % locus[1:3], b"miR-hand", b"c", b"1501", b"1522", b"+", b"1.0", b"1", b"0", b"22", b"1513", b"down", b"0"]
    assert f[13:19] == [b"16", b"16", _p16(), b"%d" % (8 * 8), b"%d" % (8 * 8), b"1"]
    assert f[19] == b"UGGACUGAAGGGAGCUCCUUCU" and f[20] == b"|" * 17 + b"x" + b"|" * 4 and f[21][17:18] == b"U"
    assert summ == [[b"c:%d-%d" % locus[1:3], b"1", b"1", b"miR-hand", b"down", b"0", _p16()]]


def test_hand_example_minus_transcript_and_up():
    rows, _, o, cut, r, locus = _hand(1, 0)
    assert len(rows) == 1 and cut == o + 10 and r == cut - 21 + 3
    assert rows[0][3:7] == [b"1501", b"1522", b"-", b"1.0"] and rows[0][10:19] == [b"%d" % cut, b"down", b"0", b"16", b"16", _p16(), b"64", b"64", b"1"]
    rows, _, o, cut, r, locus = _hand(0, 1)
    assert len(rows) == 1 and rows[0][5] == b"+" and rows[0][10:16] == [b"1513", b"up", b"0", b"16", b"16", _p16()]
    rows, _, o, cut, r, locus = _hand(1, 1)
    assert len(rows) == 1 and rows[0][5] == b"-" and rows[0][11:16] == [b"up", b"0", b"16", b"16", _p16()]


def test_formatting_of_the_module_equals_the_restatement():
    """triggers.format_outputs on the trigger rows the restatement finds: the module's writer and the restatement's give the same bytes."""
    Lp, m, alpha, K, D, flank, drift = grid_cases()[1]
    case = make_case(7, Lp, m, flank)
    kw = dict(Lp=Lp, m=m, alpha=alpha, K=K, D=D, flank=flank, drift=drift)
    tsv, summ = restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    loci = ["%s:%d-%d" % r[:3] for r in case["rows"]]
    names = [n for n, _ in case["mirnas"]]
    from mir_prefer_amd.capi import TRIGGER_DTYPE
    trig = np.zeros(len(lines_of(tsv)), TRIGGER_DTYPE)
    for i, f in enumerate(lines_of(tsv)):
        half = int(Fraction(f[6].decode()) * 2)
        trig[i] = (loci.index(f[0].decode()), names.index(f[1]), half, f[5] == b"-", f[11] == b"up", int(f[12]), int(f[13]), int(f[14]), int(f[3]) - 1,
                   int(f[16]), int(f[17]))
    counts = [int(f[1]) for f in lines_of(summ)]
    mirnas = triggers.parse_mirnas(case["mirna_fasta"])
    assert [(n, list(c)) for n, c in mirnas] == [(n, list(c)) for n, c in case["mirnas"]]
    got = triggers.format_outputs(case["rows"], mirnas, dict(zip(NAMES, case["seqs"])), trig, counts, Lp, phasing.Hypergeom(m, Lp))
    assert got == (tsv, summ) and len(trig) > 5


# ---------------------------------------------------------------------------------------------------- the phas.tsv reader
def test_parse_phas():
    good = phasing.HEADER + b"chr1\t10\t366\t8\t10\t16\t16\t1.0e-30\t50\t50\n" + b"c 2\t5\t9\t1\t7\t1\t1\t1.000e+00\t1\t1\n"
    assert triggers.parse_phas(good) == [("chr1", 10, 366, 10), ("c 2", 5, 9, 7)]
    assert triggers.parse_phas(phasing.HEADER) == []
    for bad, line in ((good.replace(b"contig", b"Contig"), 1), (b"", 1), (good + b"chr1\t1\t2\n", 4), (good + b"\n", 4),
                      (good.replace(b"\t366\t", b"\tx\t"), 2), (good + b"chr1\t1\t2\t1\t1\t1\t1\t1\t1\t1\t1\n", 4)):
        with pytest.raises(ValueError) as e:
            triggers.parse_phas(bad, "p.tsv")
        assert str(e.value).startswith("p.tsv: line %d: " % line), bad
    rows = triggers.parse_phas(good)
    triggers.check_loci(rows, {"chr1": 366, "c 2": 9})
    for lens, line in (({"chr1": 365, "c 2": 9}, 2), ({"chr1": 366}, 3)):
        with pytest.raises(ValueError) as e:
            triggers.check_loci(rows, lens, "p.tsv")
        assert str(e.value).startswith("p.tsv: line %d: " % line)
    for row in (("chr1", 0, 5, 1), ("chr1", 6, 5, 6)):
        with pytest.raises(ValueError):
            triggers.check_loci([row], {"chr1": 366})


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.triggers"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _files(tmp_path):
    (tmp_path / "m.fa").write_bytes(b">m\nUGGACUGAAGGGAGCUCCUUCU\n")
    (tmp_path / "g.fa").write_bytes(b">c1 x\n" + b"ACGT" * 100 + b"\n>c2\n" + b"A" * 50 + b"\n")
    (tmp_path / "p.tsv").write_bytes(phasing.HEADER + b"c1\t10\t366\t8\t10\t16\t16\t1.0e-30\t50\t50\n")
    (tmp_path / "a.sam").write_bytes(b"@HD\tVN:1.0\n@SQ\tSN:c1\tLN:400\n@SQ\tSN:c2\tLN:50\n")
    return [str(tmp_path / n) for n in ("m.fa", "g.fa", "p.tsv", "a.sam")]


def test_option_errors_exit_2_before_a_device(tmp_path):
    pos = _files(tmp_path)
    bad = [[], pos[:3], ["-l", "17"], ["-l", "31"], ["-c", "3"], ["-c", "21"], ["-p", "0"], ["-p", "1.5"], ["-p", "x"], ["-k", "0"], ["-k", "21"],
           ["-c", "4", "-k", "9"], ["-d", "0"], ["-d", str(1 << 31)], ["-s", "8.5"], ["-s", "0.25"], ["-s", "-1"], ["--flank", "-1"], ["--flank", "2001"],
           ["-w", "-1"], ["-w", "3"], ["--device", "-1"], ["-o", ""], ["-x"]]
    for args in bad:
        r = run_cli(args + pos if args and args != pos[:3] else args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.triggers*"))
    o = triggers.parse_args(["-l", "24", "-c", "20", "-p", "1", "-k", "40", "-d", "5", "-s", "8", "--flank", "2000", "-w", "2"] + pos)
    assert (o[0].length, o[0].cycles, o[5], o[0].min_phased, o[0].min_depth, o[6], o[0].flank, o[0].drift) == (24, 20, Fraction(1), 40, 5, 16, 2000, 2)
    o = triggers.parse_args(["-l", "18", "-c", "4", "-k", "1", "-s", "0", "--flank", "0", "-w", "0"] + pos)
    assert (o[0].length, o[0].cycles, o[6], o[0].flank, o[7]) == (18, 4, 0, 0, str(tmp_path / "p"))
    assert triggers.parse_args(pos)[5:] == (Fraction(1, 1000), 8, str(tmp_path / "p"))
    assert triggers.output_names("x.phas") == ["x.phas.triggers.tsv", "x.phas.triggers.summary.tsv"] and triggers.output_base("a.txt") == "a.txt"


def test_file_refusals_exit_255_and_leave_no_output(tmp_path):
    pos = _files(tmp_path)
    outs = triggers.output_names(str(tmp_path / "p"))
    good = (tmp_path / "p.tsv").read_bytes()
    cases = [(good.replace(b"contig\t", b"Contig\t"), "line 1: "), (good + b"c1\t1\t2\n", "line 3: "), (good + b"c9\t1\t2\t1\t1\t1\t1\t1\t1\t1\n", "line 3: unknown contig c9"),
             (good.replace(b"\t366\t", b"\t401\t"), "line 2: the locus 10-401 does not lie in 1..400 of contig c1"),
             (good + b"c2\t7\t5\t1\t1\t1\t1\t1\t1\t1\n", "line 3: "), (good + b"c2\t0\t5\t1\t1\t1\t1\t1\t1\t1\n", "line 3: ")]
    for data, why in cases:
        (tmp_path / "p.tsv").write_bytes(data)
        for p in outs:
            open(p, "wb").write(b"stale\n")
        r = run_cli(pos, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), (why, r.stderr.decode())
        assert not any(os.path.exists(p) for p in outs)
    (tmp_path / "p.tsv").write_bytes(good)
    for i in range(4):
        args = list(pos)
        args[i] = str(tmp_path / "nope")
        r = run_cli(args, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope does not exist" in r.stderr.decode()


def test_headers():
    assert triggers.HEADER == HEADER and triggers.SUMMARY_HEADER == SUMMARY_HEADER
    assert HEADER.count(b"\t") == 21 and SUMMARY_HEADER.count(b"\t") == 6

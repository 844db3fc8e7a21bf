"""Host tests of the target-mimic search (python -m mir_prefer_amd.mimics): the two restatements of tests/mimic_restatement.py agree
on seeded random inputs in which every (strand, loop position) occurs; hand-made cases with a 21-nt miRNA without equal neighbours pin the
placements, the loop lengths, the seed and closing-pair rules, the -n boundary, the tie, the blocks, the contig edges, -k, -b and the order; the
command line's option errors exit 2 without a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.mimic_restatement import (ACGT, CODE, HEADER, LOOPS, clean_mirna, loops_seen, mimic_text, partner, plant_mimic, restate, restate_files,
                                     seed_stats)
from tests.test_targets_bulge_cpu import MIX
from tests.test_targets_cpu import MCODE, ROOT, parse_mirnas, write_fasta

COMP = bytes.maketrans(b"ACGU", b"UGCA")
FWD = {0: bytes.maketrans(b"ACGU", b"ACGT"), 1: bytes.maketrans(b"ACGU", b"TGCA")}       # target-strand letter -> forward letter


def forward_loop(ys, strand):
    """The forward text of loop bases given on the target strand in column order (3'->5')."""
    return ys.translate(FWD[1]) if strand else ys.translate(FWD[0])[::-1]


def unpairing(mirna, P, G):
    """Loop bases on the target strand, in column order, that fix the placement at P: were the loop moved down by d = 1, 2, its base G - d would
    close it opposite position P - d + 1; moved up by d, its base d - 1 opposite position P + d.  Each of them is a base that pairs with none of
    the positions it could meet (no Watson-Crick pair, no G:U), so every other placement has a mismatch at a closing pair."""
    meets = {g: set() for g in range(G)}
    for d in (1, 2):
        meets[G - d].add(mirna[P - d])
        meets[d - 1].add(mirna[P + d - 1])
    pairs = {ord("A"): b"U", ord("C"): b"G", ord("G"): b"CU", ord("U"): b"AG"}
    return bytes(next(y for y in b"ACGU" if all(y not in pairs[m] for m in meets[g])) for g in range(G))


def set_pair(site, strand, P, G, L, i, y):
    """The forward site text with the target-strand base opposite miRNA position i replaced by y (A C G U)."""
    s = bytearray(site)
    s[partner(L, G, 0, strand, P, i)] = y.translate(FWD[strand])[0]
    return bytes(s)


def _rows(mirna, target, **kw):
    """one miRNA against one target text under both restatements -> the rows split at tabs"""
    mirnas = parse_mirnas(b">m\n" + mirna + b"\n")
    codes = CODE[np.frombuffer(target, dtype=np.uint8)]
    got = restate(mirnas, ["t"], [codes], plain=True, **kw)
    assert got == restate(mirnas, ["t"], [codes], **kw)
    assert got.startswith(HEADER)
    return [ln.split(b"\t") for ln in got.split(b"\n")[1:-1]]


def _site(strand, P, G=3, mirna=MIX):
    return mimic_text(mirna, strand, P, forward_loop(unpairing(mirna, P, G), strand))


# ---------------------------------------------------------------------------------------------------- the restatements agree
@pytest.mark.parametrize("seed,G", [(1, 3), (2, 2), (3, 6)])
def test_the_two_restatements_agree_and_every_loop_position_occurs(seed, G):
    rng = np.random.RandomState(seed)
    mirs = [bytes(b"ACGU"[c] for c in rng.randint(0, 4, L)) for L in (12, 17, 21, 24, 32)]
    outside = bytearray(mirs[2]); outside[14] = ord("N")                  # an unknown letter at position 15: a mismatch
    inside = bytearray(mirs[3]); inside[4] = ord("R")                     # and one at position 5: no usable seed, no site
    mirs += [bytes(outside), bytes(inside), mirs[1].replace(b"U", b"t").replace(b"A", b"a")]
    text = bytearray(ACGT[rng.randint(0, 4, 2300)].tobytes())
    at = 10
    for m in mirs:
        for strand in (0, 1):
            for P in LOOPS:
                if plant_mimic(rng, text, m.replace(b"N", b"A").replace(b"R", b"A"), strand, P, G, subs=(0, 2), at=at) is not None:
                    at += 45
    assert at < 2240
    text[3:7] = b"NNNN"
    text[2280] = ord("R")
    text[400:800] = text[400:800].lower()
    seqs = [CODE[np.frombuffer(bytes(text[:1200]), dtype=np.uint8)], CODE[np.frombuffer(bytes(text[1200:]), dtype=np.uint8)]]
    mirnas = parse_mirnas(b"".join(b">m%d x\n%s\n" % (i, m) for i, m in enumerate(mirs)))
    for kw in (dict(n=3, both=True), dict(n=0), dict(n=6, both=True, k=2), dict(n=6)):
        got = restate(mirnas, ["a", "b"], seqs, G=G, plain=True, **kw)
        assert got == restate(mirnas, ["a", "b"], seqs, G=G, **kw)
        if kw == dict(n=3, both=True):
            assert loops_seen(got) == {(s, P) for s in (b"+", b"-") for P in LOOPS}
            by = {ln.split(b"\t")[0] for ln in got.split(b"\n")[1:-1]}
            assert b"m5 x" in by and b"m6 x" not in by and b"m7 x" in by       # unknown letter outside / inside the seed; lower case and T
    assert seed_stats(mirnas, seqs, True)[0] == 1


# ---------------------------------------------------------------------------------------------------- hand-made cases
@pytest.mark.parametrize("G", [2, 3, 6])
@pytest.mark.parametrize("strand", [0, 1])
def test_perfect_mimic_at_every_loop_position(strand, G):
    L = len(MIX)
    for P in LOOPS:
        ys = unpairing(MIX, P, G)
        rows = _rows(MIX, b"GG" + _site(strand, P, G) + b"GGG", n=0, G=G, both=True)
        assert len(rows) == 1, (P, rows)
        r = rows[0]
        assert r[:8] == [b"m", b"t", b"3", b"%d" % (2 + L + G), b"-" if strand else b"+", b"0", b"0", b"0"]
        assert r[8] == MIX[:P] + b"-" * G + MIX[P:]
        assert r[9] == b"|" * P + b"-" * G + b"|" * (L - P)
        assert r[10] == MIX[:P].translate(COMP) + ys + MIX[P:].translate(COMP)
        assert r[11] == b"%d" % P
        assert _rows(MIX, b"GG" + _site(strand, P, G) + b"GGG", n=6, G=G, both=bool(1 - strand)) == ([] if strand else rows)


@pytest.mark.parametrize("strand", [0, 1])
def test_seed_takes_watson_crick_pairs_only(strand):
    L = len(MIX)
    assert MIX[2:3] == b"G" and MIX[4:5] == b"U"
    for P in LOOPS:
        site = _site(strand, P)
        for i, y in ((3, b"U"), (5, b"G"), (8, b"A"), (2, b"A")):          # G:U at 3 and 5, mismatches at 8 and 2
            assert _rows(MIX, b"GG" + set_pair(site, strand, P, 3, L, i, y) + b"GG", n=6, both=True) == []
        rows = _rows(MIX, b"GG" + set_pair(site, strand, P, 3, L, 1, b"G") + b"GG", n=6, both=True)          # position 1 is outside the seed
        assert len(rows) == 1 and rows[0][5:8] == [b"1", b"0", b"1"] and rows[0][9][:2] == b"o|"


@pytest.mark.parametrize("strand", [0, 1])
def test_closing_pairs_are_not_mismatches(strand):
    L = len(MIX)
    assert MIX[8:12] == b"GUCA"
    wrong = {ord("G"): b"A", ord("U"): b"C", ord("C"): b"A", ord("A"): b"G"}
    for P in LOOPS:
        site = _site(strand, P)
        for i in (P, P + 1):
            assert _rows(MIX, b"GG" + set_pair(site, strand, P, 3, L, i, wrong[MIX[i - 1]]) + b"GG", n=6, both=True) == [], (P, i)
    site = _site(strand, 9)                                               # positions 9 = G and 10 = U: a G:U closes the loop
    for i, y in ((9, b"U"), (10, b"G")):
        rows = _rows(MIX, b"GG" + set_pair(site, strand, 9, 3, L, i, y) + b"GG", n=1, both=True)
        assert len(rows) == 1 and rows[0][5:8] == [b"1", b"0", b"1"] and rows[0][11] == b"9"
        assert rows[0][9] == (b"|" * 8 + b"o---|" if i == 9 else b"|" * 9 + b"---o") + b"|" * 11


@pytest.mark.parametrize("strand", [0, 1])
def test_imperfect_boundary(strand):
    L = len(MIX)
    assert MIX[13:14] == b"G" and MIX[15:16] == b"U" and MIX[17:18] == b"G" and MIX[19:20] == b"A"
    site = _site(strand, 10)
    for i, y in ((14, b"U"), (16, b"G"), (18, b"A")):                      # two G:U and a mismatch
        site = set_pair(site, strand, 10, 3, L, i, y)
    rows = _rows(MIX, b"CC" + site + b"CC", n=3, both=True)
    assert len(rows) == 1 and rows[0][5:8] == [b"3", b"1", b"2"]
    assert rows[0][9] == b"|" * 10 + b"---" + b"|||o|o|x|||"
    assert _rows(MIX, b"CC" + site + b"CC", n=2, both=True) == []
    four = set_pair(site, strand, 10, 3, L, 20, b"C")
    assert _rows(MIX, b"CC" + four + b"CC", n=3, both=True) == []
    rows = _rows(MIX, b"CC" + four + b"CC", n=4, both=True)
    assert len(rows) == 1 and rows[0][5:8] == [b"4", b"2", b"2"]


@pytest.mark.parametrize("strand", [0, 1])
def test_tie_takes_the_smallest_loop_position(strand):
    """A loop whose last bases pair with positions 10 and 11 can stand after position 9, 10 or 11 at the same cost: 9 is written."""
    L = len(MIX)
    ys = b"A" + MIX[9:11].translate(COMP)                                  # columns 12..14 of the P = 11 site
    site = mimic_text(MIX, strand, 11, forward_loop(ys, strand))
    rows = _rows(MIX, b"CC" + site + b"CC", n=0, both=True)
    assert len(rows) == 1 and rows[0][11] == b"9" and rows[0][5] == b"0"
    assert rows[0][8] == MIX[:9] + b"---" + MIX[9:]
    assert rows[0][10] == MIX[:9].translate(COMP) + MIX[9:11].translate(COMP) + b"A" + MIX[9:].translate(COMP)
    ys = b"AC" + MIX[10:11].translate(COMP)                                # only position 11 pairs again: 10 and 11 tie
    rows = _rows(MIX, b"CC" + mimic_text(MIX, strand, 11, forward_loop(ys, strand)) + b"CC", n=0, both=True)
    assert len(rows) == 1 and rows[0][11] == b"10"


def test_ambiguous_base_in_the_loop_blocks_the_site():
    for strand in (0, 1):
        for letter in (b"N", b"R", b"n"):
            s = bytearray(_site(strand, 10))
            s[partner(21, 3, 0, strand, 10, 11) + (1 if strand == 0 else -1)] = letter[0]          # the loop base next to position 11's partner
            assert _rows(MIX, b"CC" + bytes(s) + b"CC", n=6, both=True) == []
        assert len(_rows(MIX, b"cc" + _site(strand, 10).lower() + b"CC", n=0, both=True)) == 1


def test_contig_edges(tmp_path):
    site = _site(0, 10)
    write_fasta(tmp_path / "m.fa", [("m", MIX)])
    write_fasta(tmp_path / "t.fa", [("whole", site), ("short5", site[1:]), ("short3", site[:-1]), ("left", b"CC" + site[:12]), ("right", site[12:] + b"CC"),
                                    ("again", _site(1, 9))])
    got = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, both=True)
    assert [ln.split(b"\t")[1:6] for ln in got.split(b"\n")[1:-1]] == [[b"whole", b"1", b"24", b"+", b"0"], [b"again", b"1", b"24", b"-", b"0"]]
    assert got == restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, both=True, plain=True)


def test_max_sites_strands_and_order(tmp_path):
    rng = np.random.RandomState(5)
    mirs = [bytes(b"ACGU"[c] for c in rng.randint(0, 4, L)) for L in (19, 21, 23)]
    texts = [bytearray(ACGT[rng.randint(0, 4, 700)].tobytes()) for _ in range(2)]
    for t in texts:
        at = 5
        for m in mirs:
            for strand in (0, 1):
                for P in LOOPS:
                    plant_mimic(rng, t, m, strand, P, 3, subs=(0, 3), at=at)
                    at += 35
    write_fasta(tmp_path / "t.fa", [("zz", bytes(texts[0])), ("aa", bytes(texts[1]))])
    write_fasta(tmp_path / "m.fa", [("m%d" % i, m) for i, m in enumerate(mirs)])
    full = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, both=True).split(b"\n")[1:-1]
    rows = [ln.split(b"\t") for ln in full]
    order = {b"zz": 0, b"aa": 1}                                          # file order, not name order
    keys = [(int(r[0][1:]), int(r[5]), order[r[1]], int(r[2]), r[4] == b"-") for r in rows]
    assert keys == sorted(keys) and len(set(k[1] for k in keys)) >= 3 and {k[2] for k in keys} == {0, 1}
    for k in (1, 2, 5):
        got = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, both=True, k=k).split(b"\n")[1:-1]
        want = []
        for i in range(3):
            want += [ln for ln in full if ln.startswith(b"m%d\t" % i)][:k]
        assert got == want and len(got) == 3 * k
        assert got == restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6, both=True, k=k, plain=True).split(b"\n")[1:-1]
    plus = restate_files(tmp_path / "m.fa", [tmp_path / "t.fa"], n=6).split(b"\n")[1:-1]
    assert plus == [ln for ln in full if ln.split(b"\t")[4] == b"+"] and 0 < len(plus) < len(full)


def test_generators():
    assert clean_mirna(b"acgTu") == b"ACGUU" and clean_mirna(b"ACGN") is None
    assert mimic_text(MIX, 1, 10, b"GGG") == MIX[:10].replace(b"U", b"T") + b"GGG" + MIX[10:].replace(b"U", b"T")
    assert list(MCODE[np.frombuffer(MIX, dtype=np.uint8)][1:8]) == [1, 2, 0, 3, 2, 1, 0]


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.mimics"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    m, t = tmp_path / "m.fa", tmp_path / "t.fa"
    m.write_bytes(b">m\n" + MIX + b"\n")
    t.write_bytes(b">t\nACGT\n")
    bad = [[], [str(m)], ["-n", "7", str(m), str(t)], ["-n", "-1", str(m), str(t)], ["-n", "x", str(m), str(t)], ["-l", "1", str(m), str(t)],
           ["-l", "7", str(m), str(t)], ["-l", "2.5", str(m), str(t)], ["-k", "-1", str(m), str(t)], ["--device", "-1", str(m), str(t)],
           ["-o", "", str(m), str(t)], ["-x", str(m), str(t)]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "m.fa").write_bytes(b">m\n" + MIX + b"\n")
    (tmp_path / "m.fa.mimics.tsv").write_bytes(b"stale\n")
    r = run_cli([str(tmp_path / "m.fa"), str(tmp_path / "nope.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.fa" in r.stderr.decode()
    r = run_cli([str(tmp_path / "nope.fa"), str(tmp_path / "m.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ")


def test_helpers_of_the_command_line(capsys):
    from mir_prefer_amd import mimics
    assert mimics.output_name("d/x_miRNA.mature.fa") == "d/x_miRNA.mature.fa.mimics.tsv"
    o, m, t, out = mimics.parse_args(["m.fa", "a.fa"])
    assert (m, t, out, o.max_imperfect, o.loop_length, o.both_strands, o.max_sites, o.device) == ("m.fa", ["a.fa"], "m.fa.mimics.tsv", 3, 3, None, 0, 0)
    o, m, t, out = mimics.parse_args(["-n", "6", "-l", "2", "-b", "-k", "7", "-o", "x.tsv", "m.fa", "a.fa", "b.fa"])
    assert (t, out, o.max_imperfect, o.loop_length, o.both_strands, o.max_sites) == (["a.fa", "b.fa"], "x.tsv", 6, 2, True, 7)
    with pytest.raises(SystemExit) as e:
        mimics.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--max-imperfect", "--loop-length", "--both-strands", "--max-sites", "--output", "--device"):
        assert opt in text

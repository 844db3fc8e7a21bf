"""Host tests of `align --tail` (DESIGN.md §12 "Tails"): the worked examples of the definition through the tests' brute-force restatement
(tests/tail_restatement.py), with the expected record lines and a summary file written by hand, and the option errors of the command, each with its
message and status 2 and without opening a device.  The GPU tests (test_align_tail_gpu.py) compare the device output with the restatement."""
import numpy as np
import pytest

from tests.tail_restatement import tail_align, tailed_hits
from tests.test_align_cpu import CODE, brute_hits

CONTIG = b"ACGTTGCAAGGCTTACCGATGGA"


def _codes(s):
    return CODE[np.frombuffer(s, dtype=np.uint8)]


def _rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def _run(reads, T=2, M=16, **kw):
    seqs = [_codes(CONTIG)]
    reads = [(q, _codes(s)) for q, s in reads]
    hits = brute_hits(seqs, reads, vmax=3)
    return tail_align(["c"], seqs, reads, hits, kw.pop("v", 0), kw.pop("k", 20), T=T, M=M, **kw)


def _records(sam):
    return [ln for ln in sam.decode().splitlines() if not ln.startswith("@")]


def test_worked_examples_of_the_definition():
    third = _rc(b"TTGCAAGGCTTACCGATG") + b"A"
    assert third == b"CATCGGTAAGCCTTGCAAA"
    sam, tsv, st, info = _run([("s_r0_x7", b"GTTGCAAGGCTTACCGATTT"), ("s_r1_x2", b"GTTGCAAGGCTTACCGATGT"), ("s_r2_x1", third)])
    assert _records(sam) == [
        "s_r0_x7\t0\tc\t3\t255\t18M2S\t*\t0\t0\tGTTGCAAGGCTTACCGATTT\tIIIIIIIIIIIIIIIIIIII\tXA:i:0\tMD:Z:18\tNM:i:0\tXT:Z:TT",
        "s_r1_x2\t0\tc\t3\t255\t19M1S\t*\t0\t0\tGTTGCAAGGCTTACCGATGT\tIIIIIIIIIIIIIIIIIIII\tXA:i:0\tMD:Z:19\tNM:i:0\tXT:Z:T",
        "s_r2_x1\t16\tc\t4\t255\t1S18M\t*\t0\t0\tTTTGCAAGGCTTACCGATG\tIIIIIIIIIIIIIIIIIII\tXA:i:0\tMD:Z:18\tNM:i:0\tXT:Z:A",
    ]
    assert tsv == b"tail\tlength\treads\tdepth\nA\t1\t1\t1\nT\t1\t1\t2\nTT\t2\t1\t7\n"
    assert st == dict(reads=3, aligned=3, unaligned=0, suppressed=0, records=3, tailed=3, tail_suppressed=0)
    assert [i["t"] for i in info] == [2, 1, 1]


def test_trimmed_records_hold_the_templated_part():
    third = _rc(b"TTGCAAGGCTTACCGATG") + b"A"
    sam, tsv, _, _ = _run([("s_r0_x7", b"GTTGCAAGGCTTACCGATTT"), ("s_r2_x1", third)], trim=True)
    assert _records(sam) == [
        "s_r0_x7\t0\tc\t3\t255\t18M\t*\t0\t0\tGTTGCAAGGCTTACCGAT\tIIIIIIIIIIIIIIIIII\tXA:i:0\tMD:Z:18\tNM:i:0\tXT:Z:TT",
        "s_r2_x1\t16\tc\t4\t255\t18M\t*\t0\t0\tTTGCAAGGCTTACCGATG\tIIIIIIIIIIIIIIIIII\tXA:i:0\tMD:Z:18\tNM:i:0\tXT:Z:A",
    ]
    assert tsv == b"tail\tlength\treads\tdepth\nA\t1\t1\t1\nTT\t2\t1\t7\n"


def test_summary_rows_are_ordered_by_length_then_letters_and_sum_depths():
    body = b"GTTGCAAGGCTTACCGAT"                                  # c[2:20], followed by G G A in the contig
    reads = [("s_r0_x5", body + b"TT"), ("s_r1_x3", body + b"TN"), ("s_r2_x4", body + b"C"), ("s_r3_x6", body + b"A"), ("s_r4", body + b"A"),
             ("s_r5_x99999999999", body + b"TT"), ("s_r6_x2", body + b"N"), ("s_r7_x8", body), ("s_r8_x9", b"ACGTACGTACGTACGTACGT")]
    sam, tsv, st, info = _run(reads)
    assert tsv == (b"tail\tlength\treads\tdepth\nA\t1\t2\t7\nC\t1\t1\t4\nN\t1\t1\t2\nTT\t2\t2\t6\nTN\t2\t1\t3\n")      # T before N
    assert st["tailed"] == 7 and st["aligned"] == 8 and st["unaligned"] == 1 and st["records"] == 9
    assert _records(sam)[7].split("\t")[5] == "18M" and "XT:Z:" not in _records(sam)[7]           # the exact read is an end-to-end hit
    assert _records(sam)[6].endswith("XT:Z:N") and _records(sam)[8].endswith("XM:i:0")


def test_the_rules_of_the_search():
    seqs = [_codes(CONTIG)]
    body = b"GTTGCAAGGCTTACCGAT"
    # maximality: the tail's first letter equals the next genome base, so only m = 19 is a hit
    assert tailed_hits(seqs, _codes(body + b"GT"), 2, 16) == [(0, 2, 0, 19)]
    # L = M: not searched; L - M < T: the tail is at most L - M letters
    assert tailed_hits(seqs, _codes(body[:16]), 2, 16) == []
    assert tailed_hits(seqs, _codes(body[:16] + b"CC"), 8, 16) == [(0, 2, 0, 16)]
    assert tailed_hits(seqs, _codes(body[:15] + b"CCC"), 8, 16) == []
    # a read that matches to its end is no tailed hit; a letter outside ACGT may be in the tail only
    assert tailed_hits(seqs, _codes(body + b"GG"), 2, 16) == []
    assert tailed_hits(seqs, _codes(body + b"N"), 2, 16) == [(0, 2, 0, 18)]
    assert tailed_hits(seqs, _codes(b"GTTGNAAGGCTTACCGAT" + b"TT"), 2, 16) == []
    # the contig's end fails every read base: c[5:23] and one more letter
    assert tailed_hits(seqs, _codes(CONTIG[5:] + b"A"), 2, 16) == [(0, 5, 0, 18)]
    # - strand at the contig's first base
    assert tailed_hits(seqs, _codes(_rc(CONTIG[:18]) + b"G"), 2, 16) == [(0, 0, 1, 18)]
    # -m counts the stratum's hits, -k keeps the first ones: two copies of the contig
    two = [_codes(CONTIG), _codes(CONTIG)]
    reads = [("q_r0_x1", _codes(body + b"TT"))]
    hits = brute_hits(two, reads, vmax=0)
    sam, tsv, st, _ = tail_align(["a", "b"], two, reads, hits, 0, 1, T=2, M=16)
    assert [ln.split("\t")[2] for ln in _records(sam)] == ["a"] and st["tailed"] == 1
    sam, tsv, st, _ = tail_align(["a", "b"], two, reads, hits, 0, 20, m=1, T=2, M=16)
    assert _records(sam) == ["q_r0_x1\t4\t*\t0\t0\t*\t*\t0\t0\tGTTGCAAGGCTTACCGATTT\tIIIIIIIIIIIIIIIIIIII\tXM:i:2"]
    assert tsv == b"tail\tlength\treads\tdepth\n" and st["tail_suppressed"] == st["suppressed"] == 1 and st["tailed"] == 0


# ---------------------------------------------------------------------------------------------------- the command's options
@pytest.fixture
def no_device(monkeypatch):
    from mir_prefer_amd import capi

    def refuse(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(capi, "Context", refuse)


@pytest.fixture
def files(tmp_path):
    (tmp_path / "g.fa").write_text(">chr1\nACGTACGTAC\n")
    (tmp_path / "s.fa").write_text(">s_r0_x3\nACGTA\n")
    return tmp_path


@pytest.mark.parametrize("argv,msg", [
    (["--tail", "0"], "Option --tail must be between 1 and 8."),
    (["--tail", "9"], "Option --tail must be between 1 and 8."),
    (["--tail", "4", "--tail-min", "11"], "Option --tail-min must be between 12 and 1024."),
    (["--tail", "4", "--tail-min", "1025"], "Option --tail-min must be between 12 and 1024."),
    (["--tail-min", "16"], "Option --tail-min needs --tail."),
    (["--tail-trim"], "Option --tail-trim needs --tail."),
    (["--tail", "4", "--place", "u"], "Options --tail and --place cannot be combined."),
    (["--tail", "4", "--place", "r"], "Options --tail and --place cannot be combined."),
])
def test_option_errors(files, no_device, capsys, argv, msg):
    from mir_prefer_amd import align
    with pytest.raises(SystemExit) as e:
        align.main(argv + ["-r", str(files / "g.fa"), str(files / "s.fa")])
    assert e.value.code == 2
    assert "mir_prefer_amd.align: error: " + msg in capsys.readouterr().err
    assert not (files / "s.fa.sam").exists() and not (files / "s.fa.sam.tails.tsv").exists()


def test_accepted_options_and_their_defaults(files):
    from mir_prefer_amd import align
    base = ["-r", str(files / "g.fa"), str(files / "s.fa")]
    o, _ = align.parse_args(base)
    assert o.tail is None and o.tail_min is None and not o.tail_trim
    o, _ = align.parse_args(["--tail", "1"] + base)
    assert (o.tail, o.tail_min, bool(o.tail_trim)) == (1, 16, False)
    o, _ = align.parse_args(["--tail", "8", "--tail-min", "12", "--tail-trim"] + base)
    assert (o.tail, o.tail_min, bool(o.tail_trim)) == (8, 12, True)
    o, _ = align.parse_args(["--tail", "3", "--tail-min", "1024"] + base)
    assert o.tail_min == 1024


def test_help_names_the_options():
    from mir_prefer_amd import align
    text = align.make_parser().format_help()
    for opt in ("--tail=", "--tail-min=", "--tail-trim"):
        assert opt in text

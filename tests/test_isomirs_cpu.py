"""CPU tests of the isomiR counts: worked examples pinned as literals (the restatement's assignment and sums, the tail code, the
three files of isomirs.py), the native tailed tokenizer against the restatement's SAM parser on every accepted, skipped and refused form, the GFF
reader on the pipeline's and on a miRBase-style file and on each refusal, the tie rule, the struct layouts against the C header, and the option
errors of the command line, which exit 2 without importing the binding.  They need the library built but no device."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from mir_prefer_amd import capi, isomirs
from mir_prefer_amd.capi import ISO_LOCUS_DTYPE, ISO_SUM_DTYPE, ISOMIR_DTYPE
from mir_prefer_amd.synth import ALN_DTYPE
from tests import isomir_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n"


def sam_line(rid, flag, contig, pos, cigar, seq, *opts):
    return "\t".join([rid, str(flag), contig, str(pos), "255", cigar, "*", "0", "0", seq, "I" * len(seq)] + list(opts)) + "\n"


def native(paths):
    names, lens, samples, alns, tails, skipped = capi.tokenize_sams_tailed([str(p) for p in paths])
    recs = [(r[0], r[4], r[1], r[3], r[2], r[5], int(t)) for r, t in zip(alns.tolist(), tails.tolist())]
    return names, lens.tolist(), samples, recs, skipped


def as_arrays(res, n_samples):
    """A scan_plain result as Context.isomir_scan returns it."""
    iso = np.array(res["isomirs"], dtype=ISOMIR_DTYPE) if res["isomirs"] else np.zeros(0, dtype=ISOMIR_DTYPE)
    sums = np.array([tuple(s) for s in res["sums"]], dtype=ISO_SUM_DTYPE)
    lc = np.array(res["locus_counts"], dtype=np.int64).reshape(len(res["sums"]), n_samples)
    ic = np.array(res["isomir_counts"], dtype=np.int64).reshape(len(res["isomirs"]), n_samples)
    return iso, sums, lc, ic


# ---------------------------------------------------------------------------------------------------- worked examples
GFF_TWO = ("##gff-version 3\n"
           "chr1\tx\tmiRNA\t101\t121\t.\t+\t.\tID=miR_plus;Name=ath-miR1\n"
           "chr1\tx\tmiRNA\t301\t321\t.\t-\t.\tID=miR_minus\n")
G21 = "ACGTACGTACGTACGTACGTA"


def worked_sam():
    """One + locus 101..121, one - locus 301..321, max5 = 2, max3 = 4."""
    return HEAD + "".join([
        sam_line("s_r1_x10", 0, "chr1", 101, "21M", G21),                                  # canonical +
        sam_line("s_r2_x7", 16, "chr1", 301, "21M", G21),                                  # canonical -
        sam_line("s_r3_x5", 0, "chr1", 101, "19M2S", G21[:19] + "TT"),                     # + trimmed by 2, tail TT
        sam_line("s_r4_x3", 16, "chr1", 303, "2S19M", "GA" + G21[:19]),                    # - : r5 = 321, r3 = 303, d3 = -2, tail = revcomp(GA) = TC
        sam_line("s_r5_x2", 0, "chr1", 101, "20M", G21[:20], "XA:i:0", "XT:Z:a"),          # --tail-trim form: d3 = -1, tail A
        sam_line("s_r6_x1", 0, "chr1", 103, "19M", G21[:19]),                              # d5 = +2 (= max5), d3 = 0
        sam_line("s_r7_x1", 0, "chr1", 99, "23M", G21 + "AC"),                             # d5 = -2
        sam_line("s_r8_x1", 0, "chr1", 104, "18M", G21[:18]),                              # d5 = +3: counts nowhere
        sam_line("s_r9_x1", 0, "chr1", 98, "24M", G21 + "ACG"),                            # d5 = -3: counts nowhere
        sam_line("s_r10_x4", 16, "chr1", 299, "21M", G21),                                 # - : r5 = 319 -> d5 = +2, r3 = 299 -> d3 = +2
        sam_line("s_r11_x4", 16, "chr1", 301, "24M", G21 + "ACG"),                         # - : r5 = 324 -> d5 = -3: nowhere
    ])


def test_worked_example_records_assignment_and_files(tmp_path):
    (tmp_path / "a.sam").write_text(worked_sam())
    (tmp_path / "m.gff3").write_text(GFF_TWO)
    names, lens, samples, recs, skipped = R.parse_sams([str(tmp_path / "a.sam")])
    assert (names, lens, samples, skipped) == (["chr1", "chr2"], [1000, 500], ["s"], {"cigar": 0, "long_tail": 0})
    tc = R.tail_code
    assert recs == [(0, 0, 101, 21, 10, 0, 0), (0, 1, 301, 21, 7, 0, 0), (0, 0, 101, 19, 5, 0, tc("TT")), (0, 1, 303, 19, 3, 0, tc("TC")),
                    (0, 0, 101, 20, 2, 0, tc("A")), (0, 0, 103, 19, 1, 0, 0), (0, 0, 99, 23, 1, 0, 0), (0, 0, 104, 18, 1, 0, 0), (0, 0, 98, 24, 1, 0, 0),
                    (0, 1, 299, 21, 4, 0, 0), (0, 1, 301, 24, 4, 0, 0)]
    assert native([tmp_path / "a.sam"]) == (names, lens, samples, recs, skipped)
    loci = [(0, 0, 101, 121), (0, 1, 301, 321)]
    by_place = {(0, 0): [(0, 101, 121)], (0, 1): [(1, 301, 321)]}
    assert [R.assign(r, by_place, 2, 4) for r in recs] == [(0, 0, 0), (1, 0, 0), (0, 0, -2), (1, 0, -2), (0, 0, -1), (0, 2, 0), (0, -2, 0), None, None,
                                                          (1, 2, 2), None]
    res = R.scan_plain(recs, loci, 2, 4, 1)
    assert res["isomirs"] == [(0, -2, 0, 0, 1), (0, 0, -2, tc("TT"), 5), (0, 0, -1, tc("A"), 2), (0, 0, 0, 0, 10), (0, 2, 0, 0, 1),
                              (1, 0, -2, tc("TC"), 3), (1, 0, 0, 0, 7), (1, 2, 2, 0, 4)]
    #              reads canonical shift5 trim3 ext3 tailed tail_u tail_a isomirs major_reads major
    assert res["sums"] == [[19, 10, 2, 7, 0, 7, 5, 2, 5, 10, 3], [14, 7, 4, 3, 4, 3, 0, 0, 3, 7, 6]]
    assert res["stats"] == (11, 8, 33, 8)
    files, st, _ = R.restate(str(tmp_path / "m.gff3"), [str(tmp_path / "a.sam")], 2, 4)
    assert files[0] == (isomirs.TSV_HEADER +
                        "miR_plus\tath-miR1\tchr1\t101\t121\t+\t19\t10\t2\t7\t0\t7\t5\t2\t5\t0\t0\t.\t10\n"
                        "miR_minus\t.\tchr1\t301\t321\t-\t14\t7\t4\t3\t4\t3\t0\t0\t3\t0\t0\t.\t7\n").encode()
    assert files[1] == b"name\ts\nmiR_plus\t19\nmiR_minus\t14\n"
    assert files[2].split(b"\n")[:3] == [b"name\td5\td3\ttail\treads\tseq\ts", b"miR_plus\t-2\t0\t.\t1\t*\t1", b"miR_plus\t0\t-2\tTT\t5\t*\t5"]
    assert st == {"records": 11, "cigar": 0, "long_tail": 0, "kept": 2, "dropped": 0, "assigned": 8, "depth": 33, "isomirs": 8}
    # isomirs.py writes the same bytes from the arrays the device returns, with and without -g
    kept, dropped = isomirs.keep_loci(isomirs.read_gff(str(tmp_path / "m.gff3")), names, lens)
    assert dropped == 0
    assert isomirs.format_files(kept, *as_arrays(res, 1), ["s"]) == files
    genome = {"chr1": np.frombuffer(("acgtn" * 200).encode(), dtype=np.uint8), "chr2": np.zeros(500, np.uint8)}
    with_g = isomirs.format_files(kept, *as_arrays(res, 1), ["s"], genome)
    assert with_g == R.files(res, kept, ["s"], genome)
    lines = with_g[2].decode().split("\n")
    assert lines[2] == "miR_plus\t0\t-2\tTT\t5\tACGUNACGUNACGUNACGUuu\t5"            # 101..119 of (acgtn)*, then the tail
    pos, length = isomirs.footprint(kept[1], 0, -2)
    assert (pos, length) == (303, 19)
    assert lines[6].split("\t")[5] == R.placement_rna(genome["chr1"], 303, True, 19).decode() + "uc"


def test_tail_code_literals():
    assert [R.tail_code(t) for t in ("", "A", "C", "N", "AA", "TT", "NN", "AAA", "NNNNNNNN")] == [0, 1, 2, 5, 6, 24, 30, 31, 488280]
    for t in ("", "A", "N", "AA", "TT", "GATTACAN", "NNNNNNNN", "TTTTTTTT"):
        assert isomirs.tail_letters(R.tail_code(t)) == t and R.tail_of_code(R.tail_code(t)) == t
    codes = [R.tail_code(t) for t in ("A", "C", "G", "T", "N", "AA", "AC", "NN", "AAA")]
    assert codes == sorted(codes) == list(range(1, 8)) + [30, 31]                      # ordered by (length, letters A < C < G < T < N)


# ---------------------------------------------------------------------------------------------------- the tokenizer against the parser
def broad_sams(tmp_path, crlf=False):
    body_a = "".join([
        sam_line("lib_A_r1_x3", 0, "chr1", 10, "21M", G21),
        sam_line("lib_A_r2_x4", 16, "chr1", 10, "21M", G21),
        sam_line("lib_A_r3_x5", 0, "chr1", 10, "19M2S", G21[:19] + "gu"),                  # lower case and U: tail GT
        sam_line("lib_A_r4_x6", 16, "chr2", 20, "3S18M", "NAu" + G21[:18]),                # revcomp(NAT) = ATN
        sam_line("lib_A_r5_x1", 0, "chr1", 10, "2S19M", G21),                              # 5' clip on +: cigar
        sam_line("lib_A_r6_x1", 16, "chr1", 10, "19M2S", G21),                             # 5' clip on -: cigar
        sam_line("lib_A_r7_x1", 0, "chr1", 10, "10M1I10M", G21),
        sam_line("lib_A_r8_x1", 0, "chr1", 10, "10M1D11M", G21),
        sam_line("lib_A_r9_x1", 0, "chr1", 10, "10M5N11M", G21),
        sam_line("lib_A_r10_x1", 0, "chr1", 10, "21M2H", G21),
        sam_line("lib_A_r11_x1", 0, "chr1", 10, "10M1P11M", G21),
        sam_line("lib_A_r12_x1", 0, "chr1", 10, "21=", G21),
        sam_line("lib_A_r13_x1", 0, "chr1", 10, "20M1X", G21),
        sam_line("lib_A_r14_x1", 0, "chr1", 10, "2S17M2S", G21),
        sam_line("lib_A_r15_x1", 0, "chr1", 10, "M", G21),
        sam_line("lib_A_r16_x1", 0, "chr1", 10, "21", G21),
        sam_line("lib_A_r17_x1", 0, "chr1", 10, "0M", "*"),
        sam_line("lib_A_r18_x1", 0, "chr1", 10, "21M0S", G21),
        sam_line("lib_A_r19_x1", 0, "chr1", 10, "20M", G21),                               # len(SEQ) != m
        sam_line("lib_A_r20_x1", 0, "chr1", 10, "19M3S", G21),                             # len(SEQ) != m + t
        sam_line("lib_A_r21_x9", 0, "chr1", 10, "21M", "*"),                               # SEQ *: kept
        sam_line("lib_A_r22_x1", 0, "chr1", 10, "19M2S", "*"),                             # a clip with SEQ *: cigar
        sam_line("lib_A_r23_x1", 0, "chr1", 10, "12M9S", G21),                             # 9-letter tail
        sam_line("lib_A_r24_x2", 0, "chr1", 10, "13M8S", G21),                             # 8 letters: kept
        sam_line("lib_A_r25_x1", 0, "chr1", 10, "21M", G21, "NM:i:0", "XT:Z:uuA"),         # tag: TTA
        sam_line("lib_A_r26_x1", 0, "chr1", 10, "21M", G21, "XT:Z:"),                      # empty tag: no tail
        sam_line("lib_A_r27_x1", 0, "chr1", 10, "21M", G21, "XT:Z:ACGTACGTA"),             # 9-letter tag
        sam_line("lib_A_r28_x1", 16, "chr1", 10, "21M", G21, "XT:Z:AC", "XT:Z:GG"),        # the first tag; as sequenced on - too
        sam_line("lib_A_r29_x1", 0, "chr1", 10, "19M2S", G21[:19] + "CC", "XT:Z:GG"),      # a clip: the tag is ignored
        sam_line("lib_A_r30_x1", 4, "*", 0, "*", G21),
        sam_line("lib_A_r31_x1", 256, "chr1", 10, "21M", G21),
        sam_line("lib_A_r32_x1", 512, "chr1", 10, "21M", G21),
        sam_line("lib_A_r33_x1", 1024 + 16, "chr1", 10, "21M", G21),
        sam_line("lib_A_r34_x1", 1 + 2 + 32 + 64, "chr1", 10, "21M", G21),                 # other flag bits do not matter
        sam_line("lib_A_r35_x7", 16, "chr1", 10, "70000M", "*"),                           # m beyond 65535
        "short\tline\n",
    ])
    body_b = sam_line("other_lib_r1_x2", 16, "chr2", 5, "1S20M", G21) + sam_line("other_lib_r2_x4000000000", 0, "chr1", 2147483632, "1M", "A")
    a, b = tmp_path / "a.sam", tmp_path / "b.sam"
    text_a, text_b = HEAD + body_a, "@SQ\tSN:zzz\tLN:5\n" + body_b
    if crlf:
        text_a, text_b = text_a.replace("\n", "\r\n"), text_b.replace("\n", "\r\n")
    a.write_bytes(text_a.encode())
    b.write_bytes(text_b.encode())
    return [a, b]


@pytest.mark.parametrize("crlf", [False, True])
def test_tokenizer_equals_the_parser(tmp_path, crlf):
    paths = broad_sams(tmp_path, crlf)
    want = R.parse_sams([str(p) for p in paths])
    assert native(paths) == want
    names, lens, samples, recs, skipped = want
    tc = R.tail_code
    assert (names, lens, samples) == (["chr1", "chr2"], [1000, 500], ["lib_A", "other_lib"])
    assert skipped == {"cigar": 18, "long_tail": 2}
    assert recs == [(0, 0, 10, 21, 3, 0, 0), (0, 1, 10, 21, 4, 0, 0), (0, 0, 10, 19, 5, 0, tc("GT")), (1, 1, 20, 18, 6, 0, tc("ATN")),
                    (0, 0, 10, 21, 9, 0, 0), (0, 0, 10, 13, 2, 0, tc(G21[13:])), (0, 0, 10, 21, 1, 0, tc("TTA")), (0, 0, 10, 21, 1, 0, 0),
                    (0, 1, 10, 21, 1, 0, tc("AC")), (0, 0, 10, 19, 1, 0, tc("CC")), (0, 0, 10, 21, 1, 0, 0),
                    (1, 1, 5, 20, 2, 1, tc("T")), (0, 0, 2147483632, 1, 4000000000, 1, 0)]


@pytest.mark.parametrize("line, message", [
    (sam_line("a_r1_x1", "x", "chr1", 10, "21M", G21), "SAM flag is not a number"),
    (sam_line("a_r1_x1", 0, "chr1", "1e3", "21M", G21), "SAM position is not a number"),
    (sam_line("a_r1_x1", 0, "chr1", 2147483633, "21M", G21), "SAM position is not a number"),
    (sam_line("a_r1", 0, "chr1", 10, "21M", G21), "Read Id format is not right. Read id must be in \"samplename_rA_xN\" format."),
    (sam_line("a_r1_x1", 0, "chr9", 10, "21M", G21), "alignment refers to a sequence that is not in the @SQ header: chr9"),
    (sam_line("a_r1_x1", 0, "chr1", 10, "*", G21), "alignment without a CIGAR string"),
    (sam_line("a_r1_x1", 0, "chr1", 10, "70000M", "A" * 70000), "read longer than 65535"),
])
def test_tokenizer_refusals(tmp_path, line, message):
    p = tmp_path / "bad.sam"
    p.write_text(HEAD + sam_line("a_r0_x1", 0, "chr1", 10, "21M", G21) + line)
    for fn in (lambda: R.parse_sams([str(p)]), lambda: capi.tokenize_sams_tailed([str(p)])):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == message


def test_tokenizer_refuses_a_file_without_header_and_a_missing_file(tmp_path):
    p = tmp_path / "nohead.sam"
    p.write_text(sam_line("a_r0_x1", 0, "chr1", 10, "21M", G21))
    for fn in (lambda: R.parse_sams([str(p)]), lambda: capi.tokenize_sams_tailed([str(p)])):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == "Can not get the sequence length from the input SAM files. Make sure SAM files have headers."
    with pytest.raises(ValueError) as e:
        capi.tokenize_sams_tailed([str(tmp_path / "nope.sam")])
    assert str(e.value) == "cannot open " + str(tmp_path / "nope.sam")


def test_the_ingest_still_reads_the_same_files(tmp_path):
    """The existing ingest, which shares its header and field code with the tailed tokenizer, keeps POS and len(SEQ) as before."""
    (tmp_path / "a.sam").write_text(worked_sam())
    names, lens, samples, alns = capi.ingest_sams([str(tmp_path / "a.sam")])
    assert (names, lens.tolist(), samples) == (["chr1", "chr2"], [1000, 500], ["s"])
    assert [(r[1], r[3], r[2], r[4]) for r in alns.tolist()] == [(98, 24, 1, 0), (99, 23, 1, 0), (101, 21, 10, 0), (101, 21, 5, 0), (101, 20, 2, 0),
                                                                 (103, 19, 1, 0), (104, 18, 1, 0), (299, 21, 4, 1), (301, 21, 7, 1), (301, 24, 4, 1),
                                                                 (303, 21, 3, 1)]
    assert capi.load_library().mirp_abi_version() == capi.ABI_VERSION == 17


# ---------------------------------------------------------------------------------------------------- GFF
PIPELINE_GFF = ("chr1\tmiR-PREFeR\tmiRNA-precursor\t80\t200\t.\t+\t.\tID=miRNA-precursor_0;NAME=miRNA-precursor_0;Other=mature_expressed=y;star_expressed=y;overhangsize=2:2\n"
                "chr1\tmiR-PREFeR\tmiRNA\t101\t121\t.\t+\t.\tID=miRNA_0;NAME=miRNA_0;Other=\n"
                "chrUn\tmiR-PREFeR\tmiRNA-precursor\t10\t120\t.\t-\t.\tID=miRNA-precursor_1;NAME=miRNA-precursor_1;Other=mature_expressed=y;star_expressed=n;overhangsize=2:2\n"
                "chrUn\tmiR-PREFeR\tmiRNA\t15\t35\t.\t-\t.\tID=miRNA_1;NAME=miRNA_1;Other=\n")
MIRBASE_GFF = ("##gff-version 3\n##date 2018-3-5\n#\n# Chromosomal coordinates of miRNAs\n"
               "chr2\t.\tmiRNA_primary_transcript\t28500\t28706\t.\t+\t.\tID=MI0005394;Alias=MI0005394;Name=ath-MIR838\n"
               "\n"
               "chr2\t.\tmiRNA\t28520\t28540\t.\t+\t.\tID=MIMAT0004260;Alias=MIMAT0004260;Name=ath-miR838;Derives_from=MI0005394\n"
               "chr1\t.\tmiRNA\t78932\t78952\t.\t-\t.\tID=MIMAT0001017;Derives_from=MI0001017\n"
               "##FASTA\n>chr1\nchr1\t.\tmiRNA\t1\t2\t.\t+\t.\tID=behind_the_directive\n")


def test_gff_readers_on_both_forms(tmp_path):
    p, m = tmp_path / "p.gff3", tmp_path / "m.gff3"
    p.write_text(PIPELINE_GFF)
    m.write_text(MIRBASE_GFF)
    want_p = [("miRNA_0", "miRNA_0", "chr1", 101, 121, "+"), ("miRNA_1", "miRNA_1", "chrUn", 15, 35, "-")]
    want_m = [("MIMAT0004260", "ath-miR838", "chr2", 28520, 28540, "+"), ("MIMAT0001017", ".", "chr1", 78932, 78952, "-")]
    for mod in (isomirs, R):
        assert mod.read_gff(str(p)) == want_p and mod.read_gff(str(m)) == want_m
        assert mod.keep_loci(want_p, ["chr1", "chr2"], [1000, 500]) == (want_p[:1], 1)           # chrUn is not in the header
        assert mod.keep_loci(want_m, ["chr2", "chr1"], [28540, 78952]) == (want_m, 0)            # ending at LN is fine
        for names, lens in ((["chr2", "chr1"], [28539, 78952]), (["chr3"], [5])):                 # beyond LN; none left
            with pytest.raises(ValueError):
                mod.keep_loci(want_m, names, lens)


@pytest.mark.parametrize("text, word", [
    ("chr1\t.\tmiRNA\t10\t30\t.\t+\t.\tID=a\nchr1\t.\tmiRNA\t50\t70\t.\t+\t.\tID=a\n", "occurs twice"),
    ("chr1\t.\tmiRNA\t10\t30\t.\t+\t.\tName=a\n", "without an ID"),
    ("chr1\t.\tmiRNA\t10\t30\t.\t+\t.\tID=\n", "without an ID"),
    ("chr1\t.\tmiRNA\t31\t30\t.\t+\t.\tID=a\n", "start behind its end"),
    ("chr1\t.\tmiRNA\t0\t30\t.\t+\t.\tID=a\n", "before position 1"),
    ("chr1\t.\tmiRNA\t10\t30\t.\t.\t.\tID=a\n", "strand"),
    ("chr1\t.\tmiRNA\t10\t30\t.\t?\t.\tID=a\n", "strand"),
    ("chr1\t.\tmiRNA\t10\t30\t.\t+\t.\tID=a\nchr1\t.\tmiRNA\t10\t30\t.\t+\t.\tID=b\n", "repeats the place"),
])
def test_gff_refusals(tmp_path, text, word):
    p = tmp_path / "bad.gff3"
    p.write_text(text)
    with pytest.raises(ValueError) as e:
        isomirs.read_gff(str(p))
    assert word in str(e.value)
    with pytest.raises(ValueError):
        R.read_gff(str(p))
    ok = tmp_path / "ok.gff3"
    ok.write_text("chr1\t.\tmiRNA\t10\t30\t.\t+\t.\tID=a\nchr1\t.\tmiRNA\t10\t30\t.\t-\t.\tID=b\nchr2\t.\tmiRNA\t10\t30\t.\t+\t.\tID=c\n")
    assert len(isomirs.read_gff(str(ok))) == 3          # the same interval on the other strand or contig is another place


# ---------------------------------------------------------------------------------------------------- the tie rule
def test_tie_rule():
    def pick(loci, rec, max5=4, max3=4):
        by = {}
        for num, (tid, strand, s, e) in enumerate(loci):
            by.setdefault((tid, strand), []).append((num, s, e))
        a = R.assign(rec, by, max5, max3)
        alns = np.array([(rec[0], rec[2], 1, rec[3], rec[1], 0)], dtype=ALN_DTYPE)
        b = R.scan_numpy(alns, np.zeros(1, np.uint32), loci, max5, max3, 1)["isomirs"]
        assert ([] if a is None else [a + (0, 1)]) == b
        return a
    nested = [(0, 0, 100, 124), (0, 0, 102, 122)]
    assert pick(nested, (0, 0, 102, 21)) == (1, 0, 0)            # exact on the inner one
    assert pick(nested, (0, 0, 100, 25)) == (0, 0, 0)
    assert pick(nested, (0, 0, 101, 23)) == (0, 1, -1)           # |d5| 1 against both: then |d3| 1 against both: then the lower number
    assert pick(nested[::-1], (0, 0, 101, 23)) == (0, -1, 1)
    same5 = [(0, 0, 100, 122), (0, 0, 100, 120)]
    assert pick(same5, (0, 0, 100, 21)) == (1, 0, 0)
    assert pick(same5, (0, 0, 100, 22)) == (0, 0, -1)            # |d3| 1 against both: the lower number
    assert pick(same5, (0, 0, 100, 24)) == (0, 0, 1)
    same5m = [(0, 1, 98, 120), (0, 1, 100, 120)]                 # on -, l5 is the end
    assert pick(same5m, (0, 1, 100, 21)) == (1, 0, 0) and pick(same5m, (0, 1, 99, 22)) == (0, 0, -1)
    signs = [(0, 0, 101, 121), (0, 0, 99, 119)]                  # the record 100..120: d5 = -1, d3 = -1 against the first, +1, +1 against the second
    assert pick(signs, (0, 0, 100, 21)) == (0, -1, -1) and pick(signs[::-1], (0, 0, 100, 21)) == (0, 1, 1)
    assert pick([(0, 0, 101, 124), (0, 0, 98, 120)], (0, 0, 100, 21)) == (0, -1, -4)     # |d5| decides before |d3|
    assert pick([(0, 0, 101, 121)], (0, 1, 101, 21)) is None and pick([(0, 0, 101, 121)], (1, 0, 101, 21)) is None
    assert pick([(0, 0, 101, 121)], (0, 0, 101, 26)) is None and pick([(0, 0, 101, 121)], (0, 0, 101, 25)) == (0, 0, 4)


# ---------------------------------------------------------------------------------------------------- layouts
def test_dtypes_have_the_c_struct_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to check the struct layout with")
    structs = [("MirpIsoLocus", ISO_LOCUS_DTYPE), ("MirpIsomir", ISOMIR_DTYPE), ("MirpIsoLocusSum", ISO_SUM_DTYPE)]
    body = "".join(' printf("%%zu ", sizeof(%s));\n' % n + "".join(' printf("%%zu ", offsetof(%s, %s));\n' % (n, f) for f in d.names) for n, d in structs)
    tailed = [f for f, _ in capi.TailedSamData._fields_]
    body += ' printf("%zu ", sizeof(MirpTailedSamData));\n' + "".join(' printf("%%zu ", offsetof(MirpTailedSamData, %s));\n' % f for f in tailed)
    body += ' printf("%zu\\n", sizeof(MirpIsomirOpts));\n'
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirprefer.h"\nint main(void) {\n' + body + " return 0;\n}\n")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    want = []
    for _, d in structs:
        want += [d.itemsize] + [d.fields[f][1] for f in d.names]
    want += [ctypes.sizeof(capi.TailedSamData)] + [getattr(capi.TailedSamData, f).offset for f in tailed]
    want += [ctypes.sizeof(capi.IsomirOpts)]
    assert got == want
    assert (ISO_LOCUS_DTYPE.itemsize, ISOMIR_DTYPE.itemsize, ISO_SUM_DTYPE.itemsize) == (24, 24, 88)


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.isomirs"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_without_the_binding(tmp_path):
    sam, gff = tmp_path / "a.sam", tmp_path / "m.gff3"
    sam.write_text(HEAD)
    gff.write_text(GFF_TWO)
    s, g = str(sam), str(gff)
    bad = [[], [g], ["--max5", "-1", g, s], ["--max5", "16", g, s], ["--max5", "x", g, s], ["--max3", "-1", g, s], ["--max3", "16", g, s],
           ["--max3", "1.5", g, s], ["--device", "-1", g, s], ["-o", "", g, s], ["-g", "", g, s], ["-x", g, s]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))
    code = ("import sys\nfrom mir_prefer_amd import isomirs\ntry:\n    isomirs.main(['--max5', '16', 'm.gff3', 'a.sam'])\nexcept SystemExit as e:\n"
            "    assert e.code == 2\nassert 'mir_prefer_amd.capi' not in sys.modules and 'numpy' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr.decode()


def test_missing_input_and_refused_gff_exit_255_and_leave_no_file(tmp_path):
    sam, gff = tmp_path / "a.sam", tmp_path / "m.gff3"
    sam.write_text(HEAD)
    gff.write_text(GFF_TWO)
    stale = [tmp_path / ("a.sam.isomirs" + ext) for ext in (".tsv", ".counts.tsv", ".isomirs.tsv")]
    r = run_cli([str(gff), str(sam), str(tmp_path / "nope.sam")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.sam" in r.stderr.decode()
    r = run_cli([str(tmp_path / "nope.gff3"), str(sam)], tmp_path)
    assert r.returncode == 255 and "nope.gff3" in r.stderr.decode()
    r = run_cli(["-g", str(tmp_path / "nope.fa"), str(gff), str(sam)], tmp_path)
    assert r.returncode == 255 and "nope.fa" in r.stderr.decode()
    for p in stale:
        p.write_bytes(b"stale\n")
    gff.write_text(GFF_TWO + GFF_TWO)                   # a duplicate ID: refused before a device is opened
    r = run_cli([str(gff), str(sam)], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and "occurs twice" in r.stderr.decode()
    assert not any(p.exists() for p in stale)


def test_helpers_of_the_command_line(capsys):
    o, gff, sams, base = isomirs.parse_args(["m.gff3", "a.sam", "b.sam"])
    assert (o.max5, o.max3, o.device, o.genome, gff, sams, base) == (2, 4, 0, None, "m.gff3", ["a.sam", "b.sam"], "a.sam.isomirs")
    assert isomirs.parse_args(["-o", "x/out.tsv", "m.gff3", "a.sam"])[3] == "x/out" and isomirs.parse_args(["-o", "out", "m.gff3", "a.sam"])[3] == "out"
    assert isomirs.parse_args(["--max5", "0", "--max3", "15", "m.gff3", "a.sam"])[0].max3 == 15
    assert isomirs.output_paths("b") == ["b.tsv", "b.counts.tsv", "b.isomirs.tsv"]
    with pytest.raises(SystemExit) as e:
        isomirs.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--max5", "--max3", "--output", "--genome", "--device"):
        assert opt in text

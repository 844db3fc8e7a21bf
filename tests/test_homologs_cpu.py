"""Homolog search, the parts that need no GPU: the restatement (tests/homolog_restatement.py: brute-force Hamming scan + the
oracle's lfold / structures / maturestar + §26's selection and merge) on hand-checked cases, the condition that the planted hairpins are found by
it, and the command's option parsing, file names and formatting."""
import pytest

from mir_prefer_amd import homologs
from tests import homolog_restatement as hr

# a perfect hairpin: 32-nt arm, 11-nt loop, the arm's reverse complement; between 100 A on either side
ARM5 = "GGCTCAGGTCCAGTCGATGCCTGAGTCCAGGC"
HAIRPIN = ARM5 + "AAAAACAAAAA" + hr.revcomp(ARM5)
CONTIG = "A" * 100 + HAIRPIN + "A" * 100
KNOWN = ARM5[5:26]          # 0-based offset 105 of CONTIG


def test_pin_perfect_placement_on_each_strand():
    """The structure line is the hairpin with one dangling base on either side: 77 characters from 1-based position 100, pairs i <-> 76 - i.  Plus
    strand: the mature is [106, 127), in the line [6, 27): all paired, 5' arm; its last pair (26, 50) and first pair (6, 70) put the star with 2-nt
    overhangs at [50 + 2, 70 + 3) of the line = [152, 173).  The hairpin's reverse complement is a hairpin too, so the same sequence also lies on
    the minus strand, in the other arm: [150, 171) with the star at [104, 125)."""
    loci, stats = hr.run([(KNOWN, ["x-miR1"])], [("c1", CONTIG)], v=0)
    assert (stats["placements"], stats["passing"], stats["loci"]) == (2, 2, 2)
    plus, minus = loci
    want = {"names": ["x-miR1"], "contig": "c1", "strand": "+", "mat_s": 106, "mat_e": 127, "mature": KNOWN, "mismatches": 0, "arm": "5p",
            "star_s": 152, "star_e": 173, "star": "TCAGGCATCGACTGGACCTGA", "fold_s": 100, "fold_e": 177, "precursor": "A" + HAIRPIN + "A",
            "total_bps": 19, "total_dots": 0, "ss": "." + "(" * 32 + "." * 11 + ")" * 32 + ".", "line_len": 77, "also": []}
    assert {k: plus[k] for k in want} == want
    assert plus["star"] == hr.revcomp(CONTIG[151:172])[::-1].translate(hr.COMP)          # the star as it stands on the plus strand
    want.update(strand="-", mat_s=150, mat_e=171, star_s=104, star_e=125, precursor=hr.revcomp("A" + HAIRPIN + "A"))
    assert {k: minus[k] for k in want} == want
    assert minus["mature"] == hr.revcomp(CONTIG[149:170]) and minus["star"] == hr.revcomp(CONTIG[103:124])
    assert homologs.locus_id(plus) == "c1_100_177_+" and homologs.locus_id(minus) == "c1_100_177_-"


def test_pin_placement_across_a_contig_boundary_is_absent():
    a, b = CONTIG[:115], CONTIG[115:]          # the site [105, 126) is cut at 115
    got, _ = hr.placements([KNOWN], [("c1", a), ("c2", b)], 0, 100)
    assert got == [(0, 1, 149 - 115, 1, 0)]          # only the other arm's site, on the minus strand of the second contig
    loci, stats = hr.run([(KNOWN, ["x-miR1"])], [("c1", a), ("c2", b)], v=0)
    assert loci == [] and stats["placements"] == 1          # and that one has lost its hairpin's other arm


def test_pin_placement_over_an_n_is_absent():
    for at in (105, 115, 125):
        c = CONTIG[:at] + "N" + CONTIG[at + 1:]
        loci, stats = hr.run([(KNOWN, ["x-miR1"])], [("c1", c)], v=3)
        assert stats["placements"] == 1 and [x["strand"] for x in loci] in ([], ["-"])
    c = CONTIG[:104] + "n" + CONTIG[105:]          # beside the site: placed, and the window shows the letter as N
    loci, stats = hr.run([(KNOWN, ["x-miR1"])], [("c1", c)], v=0)
    assert stats["placements"] == 2
    assert all("N" in x["precursor"] for x in loci)


def test_pin_window_shorter_than_55_is_no_structure():
    loci, stats = hr.run([(KNOWN, ["x-miR1"])], [("tiny", CONTIG[95:145])], v=0)
    assert loci == [] and stats["placements"] == 1 and stats["no_structure"] == 1 and sum(stats["fail_codes"]) == 0


def test_restatement_scan_order_strata_and_cut():
    pal = "ACGTACGTAGCTACGTACGT"          # its own reverse complement: both strands at one offset, + before -
    assert hr.revcomp(pal) == pal
    g = "T" * 30 + pal + "T" * 30 + pal[:10] + "G" + pal[11:] + "T" * 30
    got, dropped = hr.placements([pal, "T" * 18], [("a", g), ("b", pal)], 1, 6)          # exactly 6 placements stay, the run of T is repeat-like
    assert got == [(0, 0, 30, 0, 0), (0, 0, 30, 1, 0), (0, 0, 80, 0, 1), (0, 0, 80, 1, 1), (0, 1, 0, 0, 0), (0, 1, 0, 1, 0)] and dropped == 1
    got, dropped = hr.placements([pal], [("a", g), ("b", pal)], 1, 5)                    # one more than the cut: none
    assert got == [] and dropped == 1
    got, dropped = hr.placements([pal], [("a", g), ("b", pal)], 0, 5)
    assert [x[4] for x in got] == [0, 0, 0, 0]


def test_merge_names_by_fewest_mismatches_and_lists_the_others():
    k1 = KNOWN[:3] + "A" + KNOWN[4:]          # one mismatch
    k2 = KNOWN[:9] + "T" + KNOWN[10:]         # one mismatch, later in the file
    loci, stats = hr.run([(k1, ["b-miR2"]), (KNOWN, ["a-miR1", "c-miR1"]), (k2, ["d-miR3"])], [("c1", CONTIG)], v=1)
    assert stats["placements"] == 6 and stats["loci"] == 2
    for x in loci:
        assert x["names"] == ["a-miR1", "c-miR1"] and x["mismatches"] == 0 and x["also"] == [(["b-miR2"], 1), (["d-miR3"], 1)]
    loci, _ = hr.run([(k2, ["d-miR3"]), (k1, ["b-miR2"])], [("c1", CONTIG)], v=1)
    assert loci[0]["names"] == ["d-miR3"] and loci[0]["also"] == [(["b-miR2"], 1)]          # equal mismatches: the earlier query names the locus


# ---- a condition, not a measurement: the restatement finds the planted hairpins
SEEDS = ((1, 1), (2, 1), (3, 2), (4, 3))          # (seed, v): 12 hairpins each in 20 kb


@pytest.mark.parametrize("seed,v", SEEDS)
def test_restatement_reports_three_of_four_planted(seed, v):
    contigs, queries, planted = hr.planted_genome(seed, (20000,), 12, v)
    loci, stats = hr.run(queries, contigs, v=v)
    assert 4 * hr.found(loci, contigs, planted) >= 3 * len(planted)


def test_restatement_reports_the_mixture():
    contigs, queries, planted, loci, stats = hr.mixture()
    assert len(planted) == 40 and len(queries) == 240 and sum(len(s) for _, s in contigs) == 150000
    assert hr.found(loci, contigs, planted) >= 30 and stats["loci"] >= 30
    assert stats["placements"] > stats["passing"] and sum(1 for k in stats["fail_codes"] if k) >= 3 and stats["no_structure"] > 0


# ---- conditions of the inputs of tests/test_homologs_large_gpu.py: an input that stops exercising its path of the evaluation fails here
def test_boundary_sweep_covers_every_word_boundary_on_either_arm():
    """The coverage table of the sweep (hr.coverage_gaps says what is asked and why): every boundary 32 .. 192 is straddled by, begins and ends a
    mature and a star interval of a passing placement, with the mature in either arm."""
    contigs, queries, records, n_placements = hr.boundary_sweep()
    assert len(contigs) == 6 and all(len(c) <= (600 - 26) // 2 for _, c in contigs)
    seqs = [q for q, _ in queries]
    assert len(set(seqs) | {hr.revcomp(q) for q in seqs}) == 2 * len(seqs)          # distinct, also from every reverse complement
    assert {18, 21, 26} == {len(q) for q in seqs}
    assert n_placements >= len(records) >= 1000
    assert hr.coverage_gaps(hr.boundary_coverage(records)) == []
    assert hr.coverage_gaps(hr.boundary_coverage([r for r in records if r.prime5])) != []          # the table does tell the arms apart
    assert sum(1 for r in records if r.total_dots) >= 100 and {0, 1} == {r.prime5 for r in records}


def test_thousand_nt_windows_need_the_refold_the_rerun_and_two_rounds_of_lines():
    contigs, queries, shapes = hr.thousand()
    assert 4 <= len(queries) <= 6 and len(shapes) <= 6 and all(w["letters"] == 999 for w in shapes)
    assert max(w["lines"] for w in shapes) > hr.FOLD_LINES                  # the chunk is folded again
    assert max(w["usable"] for w in shapes) > 64                            # more than one round of 64 lines to stage, and above the 48 staged at first
    assert min(w["lines"] for w in shapes) <= hr.FOLD_LINES                 # beside a window the first fold holds
    assert max(w["structures"] for w in shapes) > 64                        # the (GTGG)n window: a second round of 64 structures as well
    assert hr.within_oracle_limits(shapes)
    _, stride, _, lds = hr.natural_launch(shapes)
    assert lds <= 64 * 1024                                                 # no opt-in, text in LDS
    lines, caps = hr.global_text_caps(shapes)
    assert lines * hr.ssw_words(stride) * 8 > 160 * 1024 >= hr.eval_lds(lines, stride, caps, text_in_lds=False) and lines >= max(w["lines"] for w in shapes)


def test_fifteen_hundred_nt_windows_need_lds_between_64_and_160_kb():
    contigs, queries, shapes = hr.fifteen_hundred()
    assert 1 <= len(shapes) <= 2 and all(w["letters"] == 1499 for w in shapes) and hr.within_oracle_limits(shapes)
    max_lines, stride, caps, lds = hr.natural_launch(shapes)
    assert (max_lines, stride, caps, lds) == (223, 1504, (27, 446, 165), 80480) and 64 * 1024 < lds <= 160 * 1024


def test_widest_window_stays_within_the_oracles_lines():
    contigs, queries, shapes = hr.widest()
    assert len(shapes) == 1 and shapes[0]["letters"] == hr.WIDEST_P - 1 and hr.within_oracle_limits(shapes)
    assert shapes[0]["lines"] > 300 and hr.natural_launch(shapes)[3] > 160 * 1024          # its text lies in global memory on natural capacities


# ---- the command
@pytest.mark.parametrize("argv", [
    [], ["mature.fa"], ["-v", "4", "m.fa", "g.fa"], ["-v", "-1", "m.fa", "g.fa"], ["-P", "59", "m.fa", "g.fa"], ["-P", "3001", "m.fa", "g.fa"],
    ["-m", "0", "m.fa", "g.fa"], ["--species", "", "m.fa", "g.fa"], ["--species", "ath,,osa", "m.fa", "g.fa"], ["-o", "", "m.fa", "g.fa"],
    ["--device", "-1", "m.fa", "g.fa"], ["--fold-model", "vienna-9", "m.fa", "g.fa"], ["-v", "x", "m.fa", "g.fa"], ["--no-such-option", "m.fa", "g.fa"]])
def test_option_errors_exit_with_status_2(argv, capsys):
    with pytest.raises(SystemExit) as e:
        homologs.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_options_and_file_names():
    o, known, genomes, species, outs = homologs.parse_args(["d/mature.fa", "g1.fa", "g2.fa"])
    assert (o.max_mismatches, o.precursor_len, o.max_placements, o.fold_model, o.device) == (1, 300, 100, "vienna-2.1.2", 0)
    assert (known, genomes, species) == ("d/mature.fa", ["g1.fa", "g2.fa"], [])
    assert outs == ("d/mature.fa.homologs.tsv", "d/mature.fa.homologs.precursor.fa", "d/mature.fa.homologs.mature.fa")
    o, _, _, species, outs = homologs.parse_args(["-v", "3", "-P", "60", "-m", "1", "--species", "ath,osa", "-o", "x/out.tsv", "--fold-model", "vienna-1.8.5",
                                                  "m.fa", "g.fa"])
    assert (o.max_mismatches, o.precursor_len, o.max_placements, o.fold_model, species) == (3, 60, 1, "vienna-1.8.5", ["ath", "osa"])
    assert outs == ("x/out.tsv", "x/out.precursor.fa", "x/out.mature.fa")
    assert homologs.parse_args(["-o", "plain", "m.fa", "g.fa"])[4] == ("plain", "plain.precursor.fa", "plain.mature.fa")


def test_missing_input_is_status_255_and_leaves_no_file(tmp_path, capsys):
    known = tmp_path / "mature.fa"
    known.write_text(">a\n" + KNOWN + "\n")
    old = tmp_path / "mature.fa.homologs.tsv"
    old.write_text("from an earlier run\n")
    assert homologs.main([str(known), str(tmp_path / "missing.fa")]) == 255
    assert "Error: file " in capsys.readouterr().err
    assert old.exists()          # a missing input is refused before anything is touched, as hairpins.py does


def test_read_known():
    data = (b">ath-miR1 first\nacgu acgu\nACGUACGUAC\n>osa-miR2\n" + b"A" * 17 + b"\n>ath-miR3\n" + b"A" * 27 + b"\n>ath-miR4\nACGTACGTACGTACGTAN\n"
            b">ath-miR5 dup\nACGTACGTACGTACGTAC\r\n>zma-miR6\n" + b"C" * 26 + b"\n")
    q, n_read, skipped = homologs.read_known(data)
    assert q == [("ACGTACGTACGTACGTAC", ["ath-miR1", "ath-miR5"]), ("C" * 26, ["zma-miR6"])] and (n_read, skipped) == (6, 3)
    q, n_read, skipped = homologs.read_known(data, ["ath"])
    assert q == [("ACGTACGTACGTACGTAC", ["ath-miR1", "ath-miR5"])] and (n_read, skipped) == (4, 2)
    assert homologs.read_known(data, ["at"]) == ([], 0, 0)
    with pytest.raises(ValueError):
        homologs.read_known(b">\nACGT\n")


LOCI = [
    {"names": ["ath-miR1", "osa-miR1"], "contig": "chr1", "strand": "+", "mat_s": 106, "mat_e": 127, "mature": "AGGTCCAGTCGATGCCTGAGT", "mismatches": 0,
     "arm": "5p", "star_s": 152, "star_e": 173, "star": "TCAGGCATCGACTGGACCTGA", "fold_s": 100, "fold_e": 177, "precursor": "ACGT" * 19 + "A",
     "energy": -7360, "line_len": 77, "total_bps": 19, "total_dots": 0, "ss": "." + "(" * 32 + "." * 11 + ")" * 32 + ".",
     "also": [(["zma-miR9"], 1), (["x-miR7", "y-miR7"], 2)]},
    {"names": ["ath-miR2"], "contig": "chr1", "strand": "+", "mat_s": 150, "mat_e": 172, "mature": "TCAGGCATCGACTGGACCTGAG", "mismatches": 2, "arm": "3p",
     "star_s": 105, "star_e": 127, "star": "CAGGTCCAGTCGATGCCTGAGT", "fold_s": 100, "fold_e": 177, "precursor": "ACGT" * 19 + "A", "energy": -7360,
     "line_len": 80, "total_bps": 20, "total_dots": 1, "ss": "." + "(" * 32 + "." * 11 + ")" * 32 + ".", "also": []},
    {"names": ["ath-miR3"], "contig": "scaffold_2", "strand": "-", "mat_s": 7, "mat_e": 25, "mature": "A" * 18, "mismatches": 3, "arm": "5p", "star_s": 40,
     "star_e": 58, "star": "T" * 18, "fold_s": 1, "fold_e": 61, "precursor": "C" * 60, "energy": -5, "line_len": 60, "total_bps": 14, "total_dots": 8,
     "ss": "(" * 25 + "." * 10 + ")" * 25, "also": []},
]


def test_formatting_of_the_three_files():
    ss = "." + "(" * 32 + "." * 11 + ")" * 32 + "."
    assert homologs.table(LOCI) == (
        "known\tcontig\tstrand\tmature_start\tmature_end\tmature_seq\tmismatches\tarm\tstar_start\tstar_end\tstar_seq\tfold_s\tfold_e\tenergy\tnorm_energy\t"
        "total_bps\ttotal_dots\tstructure\talso\n"
        "ath-miR1,osa-miR1\tchr1\t+\t106\t127\tAGGTCCAGTCGATGCCTGAGT\t0\t5p\t152\t173\tTCAGGCATCGACTGGACCTGA\t100\t177\t-73.60\t-0.955844\t19\t0\t" + ss +
        "\tzma-miR9:1;x-miR7,y-miR7:2\n"
        "ath-miR2\tchr1\t+\t150\t172\tTCAGGCATCGACTGGACCTGAG\t2\t3p\t105\t127\tCAGGTCCAGTCGATGCCTGAGT\t100\t177\t-73.60\t-0.920000\t20\t1\t" + ss + "\t.\n"
        "ath-miR3\tscaffold_2\t-\t7\t25\t" + "A" * 18 + "\t3\t5p\t40\t58\t" + "T" * 18 + "\t1\t61\t-0.05\t-0.000833\t14\t8\t" + "(" * 25 + "." * 10 + ")" * 25 + "\t.\n")
    assert homologs.precursor_fasta(LOCI) == ">chr1_100_177_+\n" + "ACGT" * 19 + "A\n>scaffold_2_1_61_-\n" + "C" * 60 + "\n"
    assert homologs.mature_fasta(LOCI) == (">chr1_100_177_+ ath-miR1,osa-miR1 106_127\nAGGTCCAGTCGATGCCTGAGT\n>chr1_100_177_+ ath-miR2 150_172\n"
                                           "TCAGGCATCGACTGGACCTGAG\n>scaffold_2_1_61_- ath-miR3 7_25\n" + "A" * 18 + "\n")
    assert homologs.table([]) == homologs.HEADER and homologs.precursor_fasta([]) == "" and homologs.mature_fasta([]) == ""


def test_summary_text():
    stats = {"queries": 5, "repeat_like": 1, "placements": 9, "passing": 4, "loci": 3, "fail_codes": [0, 0, 2, 0, 1] + [0] * 8, "no_structure": 2}
    assert homologs.summary_text(8, 2, stats) == (
        "known sequences read\t8\nknown sequences skipped\t2\nqueries\t5\nqueries repeat-like\t1\nplacements\t9\nwindows folded\t9\nloci\t3\n"
        "placements without a passing structure\t5\n  FAIL_STRUCTURE_MATURE_NOT_IN_FOLD_REGION\t2\n  FAIL_STRUCTURE_MATURE_MATCH_SMALL_THAN_14\t1\n"
        "  no structure\t2\n")
    from tests import oracle_binding
    assert homologs.MS_CODES == oracle_binding.MS_CODES


def test_loci_of_cuts_the_window_on_its_strand():
    import numpy as np
    from mir_prefer_amd import capi
    recs = np.zeros(2, dtype=capi.HOMOLOG_DTYPE)
    win = "AACCGGTTAC"          # the contig's [11, 21)
    for r, strand in zip(recs, (0, 1)):
        r["query"], r["strand"], r["win_s"], r["win_e"], r["mat_s"], r["mat_e"], r["star_s"], r["star_e"], r["fold_s"], r["fold_e"] = 0, strand, 11, 21, 12, 14, 17, 19, 11, 20
        r["ss_len"], r["prime5"], r["line_len"] = 3, 1 - strand, 9
    recs[1]["text_off"], recs[1]["n_also"] = 13, 1
    text = (win + "(.)" + hr.revcomp(win) + ".).").encode()
    loci = homologs.loci_of(recs, text, np.array([[0, 2]], dtype=np.int32), [("ACGT", ["n1", "n2"])], ["c"])
    assert (loci[0]["mature"], loci[0]["star"], loci[0]["precursor"], loci[0]["ss"], loci[0]["arm"], loci[0]["also"]) == ("AC", "TT", "AACCGGTTA", "(.)", "5p", [])
    assert (loci[1]["mature"], loci[1]["star"], loci[1]["precursor"], loci[1]["ss"], loci[1]["arm"]) == ("GT", "AA", "TAACCGGTT", ".).", "3p")
    assert loci[1]["also"] == [(["n1", "n2"], 2)] and loci[1]["names"] == ["n1", "n2"]

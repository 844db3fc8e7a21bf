"""Homolog search on the device against its restatement (tests/homolog_restatement.py): records, dot-brackets, statistics and file
bytes, all by exact equality."""
import os
import random

import pytest

from mir_prefer_amd import homologs
from tests import homolog_restatement as hr
from tests.test_homologs_cpu import ARM5, CONTIG, HAIRPIN, KNOWN

pytestmark = pytest.mark.gpu
COUNTS = ("queries", "repeat_like", "placements", "passing", "loci", "fail_codes", "no_structure")


def device_run(ctx, tmp_path, queries, contigs, v=1, P=300, max_placements=100, **caps):
    """(loci, counts) of the device for the same input as hr.run."""
    path = str(tmp_path / "genome.fa")
    hr.write_fasta(path, contigs)
    ctx.align_index([path])
    recs, text, also = ctx.homolog_scan([q for q, _ in queries], max_mismatches=v, precursor_len=P, max_placements=max_placements, **caps)
    stats = ctx.homolog_last_stats()
    names, lens = ctx.align_contigs()
    assert names == [n for n, _ in contigs] and list(lens) == [len(s) for _, s in contigs]
    return homologs.loci_of(recs, text, also, queries, names), {k: stats[k] for k in COUNTS}, stats


def check(ctx, tmp_path, queries, contigs, **kw):
    caps = {k: kw.pop(k) for k in ("keys", "chunk", "fold_lines", "eval_caps") if k in kw}
    want_loci, want_stats = hr.run(queries, contigs, **kw)
    loci, counts, stats = device_run(ctx, tmp_path, queries, contigs, **kw, **caps)
    assert counts == want_stats
    assert loci == want_loci
    return loci, stats


# ---- the CPU pins, on the device
def test_pins(gpu_ctx, tmp_path):
    q = [(KNOWN, ["x-miR1"])]
    loci, _ = check(gpu_ctx, tmp_path, q, [("c1", CONTIG)], v=0)
    assert [(x["strand"], x["mat_s"], x["mat_e"], x["star_s"], x["star_e"], x["arm"]) for x in loci] == [("+", 106, 127, 152, 173, "5p"), ("-", 150, 171, 104, 125, "5p")]
    loci, _ = check(gpu_ctx, tmp_path, q, [("c1", CONTIG[:115]), ("c2", CONTIG[115:])], v=0)          # across a contig boundary
    assert loci == []
    for at in (105, 115, 125):                                                                      # over an N
        check(gpu_ctx, tmp_path, q, [("c1", CONTIG[:at] + "N" + CONTIG[at + 1:])], v=3)
    check(gpu_ctx, tmp_path, q, [("c1", CONTIG[:104] + "n" + CONTIG[105:])], v=0)                    # an N beside it
    _, stats = check(gpu_ctx, tmp_path, q, [("tiny", CONTIG[95:145])], v=0)                          # a window shorter than 55 nt
    assert stats["no_structure"] == 1


# ---- edges of the scan
def mutate(rng, s, k):
    s = list(s)
    for p in rng.sample(range(len(s)), k):
        s[p] = rng.choice([c for c in "ACGT" if c != s[p]])
    return "".join(s)


def perfect_hairpin(rng, arm_len=40):
    arm = hr.random_seq(rng, arm_len)
    return arm + hr.random_seq(rng, 12) + hr.revcomp(arm)


@pytest.mark.parametrize("v", [0, 1, 2, 3])
def test_scan_edges(gpu_ctx, tmp_path, v):
    rng = random.Random(100 + v)
    queries, body = [], []
    for L in (18, 26):          # a site with 0..3 mismatches for either length, each in a hairpin of its own
        for k in range(4):
            hp = perfect_hairpin(rng)
            queries.append((mutate(rng, hp[7:7 + L], k), ["e-miR%d-%d" % (L, k)]))
            body.append(hr.random_seq(rng, 150) + hp)
    first, last = perfect_hairpin(rng), perfect_hairpin(rng)
    queries += [(first[:21], ["e-first"]), (last[-22:], ["e-last"])]          # offset 0, and ending at the contig's last base; either on both strands
    pal = "ACGTACGTAGCTACGTACGT"                                             # reverse-palindromic: both strands at one offset
    queries.append((pal, ["e-pal"]))
    amb = hr.random_seq(rng, 20)                                             # an ambiguous base at each end of the would-be placement
    queries.append((amb, ["e-amb"]))
    main = first + "".join(body) + hr.random_seq(rng, 100) + pal + hr.random_seq(rng, 100) + "N" + amb[1:] + "TT" + amb[:-1] + "n" + "TT" + amb + hr.random_seq(rng, 90) + last
    contigs = [("short10", hr.random_seq(rng, 10)), ("main", main), ("short17", KNOWN[:17]), ("rev", hr.revcomp(main)), ("one", "A")]
    loci, stats = check(gpu_ctx, tmp_path, queries + [(KNOWN, ["x-miR1"])], contigs, v=v)
    assert stats["placements"] >= 2 * (2 * (v + 1) + 2 + 1 + 1) and len(loci) >= 2 * (v + 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_query_counts(gpu_ctx, tmp_path, n):
    contigs, queries, planted = hr.planted_genome(5, (12000,), 8, 1, n_decoys=124)
    order = list(range(len(queries)))
    random.Random(n).shuffle(order)          # the planted ones anywhere among the queries
    loci, _ = check(gpu_ctx, tmp_path, [queries[k] for k in order[:n]], contigs, v=1)
    if n == 129:
        assert len(loci) >= 8


def test_max_placements_cut(gpu_ctx, tmp_path):
    rng = random.Random(7)
    qa, qb, qc = (hr.random_seq(rng, 21) for _ in range(3))
    parts = [hr.random_seq(rng, 120)]
    for s in (qa, qa, hr.revcomp(qa), qb, qb, hr.revcomp(qb), mutate(rng, qb, 1), qc):
        parts += [s, hr.random_seq(rng, 120)]
    contigs = [("c", "".join(parts))]
    queries = [(qa, ["exactly-m"]), (qb, ["m-plus-one"]), (qc, ["single"])]
    _, stats = check(gpu_ctx, tmp_path, queries, contigs, v=1, max_placements=3)
    assert (stats["repeat_like"], stats["placements"]) == (1, 4)
    _, stats = check(gpu_ctx, tmp_path, queries, contigs, v=1, max_placements=4)
    assert (stats["repeat_like"], stats["placements"]) == (0, 8)
    _, stats = check(gpu_ctx, tmp_path, queries, contigs, v=0, max_placements=3)          # the cut counts the placements within v only
    assert (stats["repeat_like"], stats["placements"]) == (0, 7)


def test_merge_and_also(gpu_ctx, tmp_path):
    k1 = KNOWN[:3] + "A" + KNOWN[4:]
    k2 = KNOWN[:9] + "T" + KNOWN[10:]
    loci, _ = check(gpu_ctx, tmp_path, [(k1, ["b-miR2"]), (KNOWN, ["a-miR1", "c-miR1"]), (k2, ["d-miR3"])], [("c1", CONTIG)], v=1)
    assert [x["also"] for x in loci] == [[(["b-miR2"], 1), (["d-miR3"], 1)]] * 2
    loci, _ = check(gpu_ctx, tmp_path, [(k2, ["d-miR3"]), (k1, ["b-miR2"])], [("c1", CONTIG)], v=1)
    assert loci[0]["names"] == ["d-miR3"]
    longer = ARM5[5:27]          # another length at the same start: a locus of its own
    loci, _ = check(gpu_ctx, tmp_path, [(KNOWN, ["a-miR1"]), (longer, ["a-miR1-22"])], [("c1", CONTIG)], v=0)
    assert len(loci) == 4 and all(x["also"] == [] for x in loci)


# ---- edges of the windows
@pytest.mark.parametrize("P", [60, 300, 301, 400])
def test_precursor_lengths_and_clipped_flanks(gpu_ctx, tmp_path, P):
    """Both fold paths (span <= 300 and above) and, at 60, windows whose structure list is empty; the hairpin 5 nt from either contig end, in the
    middle, and in a contig that is shorter than the window."""
    contigs = [("left", "A" * 5 + HAIRPIN + "A" * 400), ("right", "C" * 400 + HAIRPIN + "A" * 5), ("mid", CONTIG + "A" * 300), ("small", "AA" + HAIRPIN + "AAA")]
    _, stats = check(gpu_ctx, tmp_path, [(KNOWN, ["x-miR1"])], contigs, v=0, P=P)
    assert stats["placements"] == 8
    if P == 60:
        assert stats["no_structure"] > 0 and stats["loci"] == 0
    else:
        assert stats["loci"] == 8


# ---- capacity: the same output however the work is split
def test_mixture_and_capacities(gpu_ctx, tmp_path):
    contigs, queries, planted, want_loci, want_stats = hr.mixture()
    loci, counts, stats = device_run(gpu_ctx, tmp_path, queries, contigs, v=2)
    assert counts == want_stats
    assert loci == want_loci
    assert len(loci) == len(want_loci) >= 30 and hr.found(loci, contigs, planted) >= 30
    assert (stats["scan_passes"], stats["chunks"], stats["folds"], stats["eval_reruns"]) == (1, 1, 1, 0)
    text = homologs.table(loci)
    for caps, seen in ((dict(keys=2), "scan_passes"), (dict(keys=40), "scan_passes"), (dict(chunk=3), "chunks"), (dict(fold_lines=3), "folds"),
                       (dict(eval_caps=(1, 2, 2)), "eval_reruns")):
        again, counts, stats = device_run(gpu_ctx, tmp_path, queries, contigs, v=2, **caps)
        assert counts == want_stats and again == loci and homologs.table(again) == text
        assert stats[seen] > {"scan_passes": 1, "chunks": 1, "folds": 1, "eval_reruns": 0}[seen], (caps, stats)
    _, _, stats = device_run(gpu_ctx, tmp_path, queries, contigs, v=2, keys=2)
    assert stats["scan_passes"] >= want_stats["placements"] // 2
    again, _, stats = device_run(gpu_ctx, tmp_path, queries, contigs, v=2, chunk=3)
    assert stats["chunks"] == (want_stats["placements"] + 2) // 3 and again == loci


def test_key_capacity_below_one_querys_placements(gpu_ctx, tmp_path):
    """A query whose placements alone exceed the key capacity goes through the plan's position ranges."""
    rng = random.Random(3)
    q = hr.random_seq(rng, 21)
    contigs = [("c", "".join(hr.random_seq(rng, 80) + (q if k % 2 else hr.revcomp(q)) for k in range(9)) + hr.random_seq(rng, 50))]
    want, _ = hr.run([(q, ["r"])], contigs, v=0)
    _, counts, stats = device_run(gpu_ctx, tmp_path, [(q, ["r"])], contigs, v=0, keys=2)
    assert counts["placements"] == 9 and stats["scan_passes"] > 5
    loci, _, _ = device_run(gpu_ctx, tmp_path, [(q, ["r"])], contigs, v=0, keys=2)
    assert loci == want


# ---- the command line end to end
def test_command_line(tmp_path, capsys):
    contigs, queries, planted = hr.planted_genome(9, (9000, 6000), 6, 1, n_decoys=20)
    known, g1, g2 = str(tmp_path / "mature.fa"), str(tmp_path / "g1.fa"), str(tmp_path / "g2.fa")
    with open(known, "w") as f:
        f.write(">ath-short\nACGUACGU\n>ath-bad\nACGTACGTACGTACGTACNN\n")
        for k, (seq, names) in enumerate(queries):
            f.write(">%s some text\n%s\n" % (names[0].replace("pln", "ath").replace("dcy", "osa"), seq.lower().replace("t", "u") if k % 2 else seq))
        f.write(">ath-again\n%s\n>zma-other\n%s\n" % (queries[0][0], queries[1][0]))
    hr.write_fasta(g1, contigs[:1])
    hr.write_fasta(g2, contigs[1:])
    with open(known, "rb") as f:
        q, n_read, skipped = homologs.read_known(f.read(), ["ath", "osa"])
    assert (len(q), n_read, skipped) == (len(queries), len(queries) + 3, 2) and q[0][1] == ["ath-miR1", "ath-again"]
    want_loci, want_stats = hr.run(q, contigs, v=1)
    assert len(want_loci) >= 6
    outs = [known + ".homologs" + e for e in (".tsv", ".precursor.fa", ".mature.fa")]
    assert homologs.main(["--species", "ath,osa", known, g1, g2]) == 0
    for path, want in zip(outs, (homologs.table(want_loci), homologs.precursor_fasta(want_loci), homologs.mature_fasta(want_loci))):
        with open(path, newline="") as f:
            assert f.read() == want
    st = dict(want_stats)
    assert capsys.readouterr().out == homologs.summary_text(n_read, skipped, st)
    # the written precursors chain into randfold as they are
    from mir_prefer_amd import randfold
    assert randfold.main(["-n", "3", outs[1]]) == 0
    with open(outs[1] + ".randfold.tsv") as f:
        assert len(f.read().splitlines()) == 1 + len({homologs.locus_id(x) for x in want_loci})
    # a refused input leaves no file, not even the earlier run's
    bad = str(tmp_path / "bad.fa")
    with open(bad, "w") as f:
        f.write(">\nACGT\n")
    assert homologs.main(["-o", outs[0], bad, g1]) == 255
    assert not any(os.path.exists(p) for p in outs)
    empty = str(tmp_path / "empty_genome.fa")
    with open(empty, "w") as f:
        f.write(">c1\nACGT\n>c1\nACGT\n")          # a duplicate contig name: the index refuses it
    assert homologs.main(["-o", outs[0], known, empty]) == 255
    assert not any(os.path.exists(p) for p in outs)
    assert "Error: " in capsys.readouterr().err

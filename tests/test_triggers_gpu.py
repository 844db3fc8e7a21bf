"""GPU tests of the miRNA triggers of PHAS loci (mirp_trigger_scan, trigger_kernels.hip): whole files against the restatements of
tests/trigger_restatement.py over the grid of tests/test_triggers_cpu.py (Lp 21 / 22 / 24, the four settings of the phasing grid, every plant) on
SAM input in three files with flagged and gapped records; a saturated region; coordinates near and past 2^31; 65,537 miRNAs; empty inputs; mirp_phase_scan
after mirp_trigger_scan; the command line in a child process and the chain reads collapse -> align -> phasing -g -> triggers."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from mir_prefer_amd import capi, phasing, triggers
from tests.test_phasing_cpu import ROOT, make_records
from tests.test_phasing_gpu import _genome, _revcomp, write_sams
from tests.test_targets_cpu import parse_mirnas, target_of_mirna
from tests.test_triggers_cpu import ACGT, LENS, NAMES, check_plants, grid_cases, lines_of, make_case
from tests.trigger_restatement import HEADER, SUMMARY_HEADER, restate_numpy, restate_plain

pytestmark = pytest.mark.gpu


def _scan(ctx, d, names, seqs, mirna_fasta, rows, order=None, **kw):
    """Writes the miRNA and genome files (the genome's contigs in `order`) and scans ctx's resident alignments."""
    (d / "m.fa").write_bytes(mirna_fasta)
    order = list(range(len(names))) if order is None else order
    _genome(d / "g.fa", [names[i] for i in order], [seqs[i] for i in order])
    return triggers.scan(ctx, str(d / "m.fa"), str(d / "g.fa"), rows, names, capi.read_fasta(str(d / "g.fa")), kw.pop("Lp"), kw.pop("m"), kw.pop("alpha"),
                         min_phased=kw.pop("K"), min_depth=kw.pop("D"), **kw)


@pytest.mark.parametrize("case_id", range(12))
def test_grid_matches_the_restatement(gpu_ctx, tmp_path, case_id):
    Lp, m, alpha, K, D, flank, drift = grid_cases()[case_id]
    case = make_case(100 + case_id, Lp, m, flank)
    rng = np.random.RandomState(case_id)
    extra = [(int(rng.randint(0, 3)), int(flag), int(rng.randint(0, 4)), int(rng.randint(1, 120)), int(rng.randint(1, 50)), Lp)
             for flag in (4, 256, 1024, 4 | 16, 256 | 16) for _ in range(10)]
    paths = [str(tmp_path / ("s%d.sam" % i)) for i in range(3)]
    write_sams(paths, NAMES, LENS, case["alns"], extra)
    n_names, n_lens, _, alns, _, _ = gpu_ctx.ingest_sams(paths)
    assert n_names == NAMES and n_lens.tolist() == LENS and len(alns) == len(case["alns"])
    kw = dict(Lp=Lp, m=m, alpha=alpha, K=K, D=D, flank=flank, drift=drift)
    tsv, summ, stats = _scan(gpu_ctx, tmp_path, NAMES, case["seqs"], case["mirna_fasta"], case["rows"], order=[3, 2, 1, 0], **kw)
    want = restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    assert (tsv, summ) == want, kw
    if case_id == 0:
        assert (flank, drift, K, D) == (100, 0, 3, 1) and restate_plain(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw) == want
    assert check_plants(case, tsv, summ, flank, drift, K) >= 9
    per = 2 * (2 * drift + 1)
    assert stats["mirnas"] == 11 and stats["windows"] == stats["sites"] * per and stats["trigger_lines"] == len(lines_of(tsv))
    assert stats["sites"] == sum(int(f[1]) for f in lines_of(summ)) and stats["records"] == int((case["alns"]["len"] == Lp).sum())
    # the edge plant: one base more of flank takes its site in
    kw["flank"] = flank + 1
    tsv1, summ1, _ = _scan(gpu_ctx, tmp_path, NAMES, case["seqs"], case["mirna_fasta"], case["rows"], **kw)
    assert (tsv1, summ1) == restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    assert any(f[1] == b"edge" and f[5] == b"+" and f[11] == b"up" and f[12] == b"0" for f in lines_of(tsv1))


def test_saturated_region(gpu_ctx, tmp_path):
    """Every coordinate of a 10 kb region occupied on both strands, sites inside: n = S, and the counting stays bounded."""
    rng = np.random.RandomState(5)
    seq = bytearray(ACGT[rng.randint(0, 4, 12000)].tobytes())
    mirs = [bytes(b"ACGU"[c] for c in rng.randint(0, 4, L)) for L in (21, 22, 24)]
    for i, o in enumerate(range(1500, 10500, 900)):
        mir = mirs[i % 3]
        seq[o:o + len(mir)] = target_of_mirna(mir.replace(b"U", b"T"), i % 2)
    rows_r = [(0, p, int(rng.randint(1, 9)), 21, s) for p in range(1000, 11000) for s in (0, 1)]
    rows_r += [(0, p, 2, 24, s) for p in range(3000, 3400) for s in (0, 1)]
    recs = make_records(rows_r)
    gpu_ctx.load_genome([("c0", np.full(12000, 65, np.uint8))])
    gpu_ctx.load_alignments(recs)
    fasta = b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(mirs))
    rows = [("c0", a, a + 699, a + 3) for a in range(1400, 10400, 900)] + [("c0", 900, 1100, 1000), ("c0", 10900, 11100, 10950)]
    for Lp, m, alpha, K, drift in ((21, 10, Fraction(1, 1000), 3, 0), (21, 20, Fraction(1), 1, 2), (24, 4, Fraction(1), 1, 1)):
        kw = dict(Lp=Lp, m=m, alpha=alpha, K=K, D=1, flank=100, drift=drift)
        tsv, summ, stats = _scan(gpu_ctx, tmp_path, ["c0"], [bytes(seq)], fasta, rows, **kw)
        assert (tsv, summ) == restate_numpy(recs, ["c0"], [bytes(seq)], parse_mirnas(fasta), rows, **kw), (Lp, m)
        if K == 1:
            f = lines_of(tsv)
            if Lp == 21:                                    # every site lies deep in the region: each of its windows holds a phased unit
                assert len(f) == stats["windows"] >= 10 * (2 * drift + 1) * 2
                assert max(int(x[13]) for x in f) == 2 * m * Lp and max(int(x[14]) for x in f) == 2 * m


def test_coordinates_near_2_31(gpu_ctx, tmp_path):
    """A contig of nearly 2^31 N and a 60 kb tail that crosses 2^31: records through load_alignments up to pos 2^31 - 1 (the largest a record
    holds), registers up to 2^31 + 1, and a site past 2^31."""
    rng = np.random.RandomState(9)
    Lp, m = 21, 10
    tail = bytearray(ACGT[rng.randint(0, 4, 60000)].tobytes())
    mirs = [bytes(b"ACGU"[c] for c in rng.randint(0, 4, L)) for L in (21, 22)]
    recs, rows = [], []
    for i, o in enumerate((1000, 9000, 20000, 41000)):
        mir, strand, side = mirs[i % 2], i % 2, i // 2
        tail[o:o + len(mir)] = target_of_mirna(mir.replace(b"U", b"T"), strand)
        r = o + 13 - Lp if strand else o + len(mir) - 9
        x = (r + (Lp if side else -(m - 1) * Lp)) if strand else (r - (m * Lp if side else 0))
        for j in range(m):
            recs += [(0, x + j * Lp, 4, Lp, 0), (0, x + j * Lp - 2, 6, Lp, 1)]
        rows.append(("big", min(o + 1, x), max(o + 30, x + m * Lp), x))
    top = max(r[1] for r in recs)
    recs.append((0, top, 3, Lp, 1))                                   # the last minus read: pos 2^31 - 1, c = 2^31 + 1
    pad = 2 ** 31 - 1 - top
    tail[50000:50021] = target_of_mirna(mirs[0].replace(b"U", b"T"), 0)   # a site past 2^31, no reads
    rows.append(("big", 49900, 50300, 50000))
    recs += [(int(rng.randint(0, 2)), int(rng.randint(300, 19000)), int(rng.randint(1, 9)), int(rng.choice([20, 21, 22])), int(rng.randint(0, 2)))
             for _ in range(2000)]
    small = make_records(recs)
    big = small.copy()
    big["pos"][big["tid"] == 0] += pad
    big = big[np.lexsort((big["pos"], big["tid"]))]
    assert int(big["pos"].max()) == 2 ** 31 - 1
    other = ACGT[rng.randint(0, 4, 20000)].tobytes()
    p = tmp_path / "big.fa"
    line = b"N" * 4095 + b"\n"
    with open(p, "wb") as f:
        f.write(b">big\n")
        left = pad
        while left >= 4095 * 16384:
            f.write(line * 16384)
            left -= 4095 * 16384
        f.write(b"N" * left + b"\n" + bytes(tail) + b"\n>other\n" + other + b"\n")
    fasta = b"".join(b">s%d\n%s\n" % (i, s) for i, s in enumerate(mirs))
    (tmp_path / "m.fa").write_bytes(fasta)
    gpu_ctx.load_genome([("big", np.full(10, 65, np.uint8)), ("other", np.full(10, 65, np.uint8))])
    gpu_ctx.load_alignments(big)
    rows_big = [(n, a + pad, b + pad, x + pad) for n, a, b, x in rows] + [("other", 500, 900, 500)]
    genome = capi.read_fasta(str(p))
    tsv, summ, stats = triggers.scan(gpu_ctx, str(tmp_path / "m.fa"), str(p), rows_big, ["big", "other"], genome, Lp, m, Fraction(1, 1000), drift=1)
    del genome
    os.unlink(p)
    want_tsv, want_summ = restate_numpy(small, ["big", "other"], [bytes(tail), other], parse_mirnas(fasta), rows + [("other", 500, 900, 500)], Lp=Lp, m=m,
                                        drift=1)

    def shift(data, cols):
        out = []
        for ln in data.split(b"\n")[1:-1]:
            f = ln.split(b"\t")
            if f[0].startswith(b"big:"):
                a, b = f[0][4:].split(b"-")
                f[0] = b"big:%d-%d" % (int(a) + pad, int(b) + pad)
                for c in cols:
                    f[c] = b"%d" % (int(f[c]) + pad)
            out.append(b"\t".join(f) + b"\n")
        return data.split(b"\n")[0] + b"\n" + b"".join(out)
    assert tsv == shift(want_tsv, (3, 4, 10)) and summ == shift(want_summ, ())
    f = lines_of(tsv)
    assert {(x[5], x[11]) for x in f} == {(b"+", b"down"), (b"-", b"down"), (b"+", b"up"), (b"-", b"up")} and max(int(x[10]) for x in f) > 2 ** 31 - 300
    assert lines_of(summ)[4][:3] == [b"big:%d-%d" % (49900 + pad, 50300 + pad), b"1", b"0"] and 49900 + pad > 2 ** 31


def test_65537_mirnas_the_last_one_the_only_trigger(gpu_ctx, tmp_path):
    """One miRNA more than a group of the site scan holds; only the last one has a site (-s 0)."""
    case = make_case(3, 21, 10, 100)
    rng = np.random.RandomState(8)
    letters = np.frombuffer(b"ACGU", np.uint8)[rng.randint(0, 4, (65536, 21))]
    m21 = dict((n, c) for n, c in case["mirnas"])[b"m21"]
    fasta = b"".join(b">x%d\n%s\n" % (i, letters[i].tobytes()) for i in range(65536)) + b">last\n" + bytes(b"ACGU"[c] for c in m21) + b"\n"
    gpu_ctx.load_genome([(n, np.full(10, 65, np.uint8)) for n in NAMES])
    gpu_ctx.load_alignments(case["alns"])
    kw = dict(Lp=21, m=10, alpha=Fraction(1, 1000), K=3, D=1, flank=100, drift=1, max_half_score=0)
    tsv, summ, stats = _scan(gpu_ctx, tmp_path, NAMES, case["seqs"], fasta, case["rows"], **kw)
    kw["max_half"] = kw.pop("max_half_score")
    want = restate_numpy(case["alns"], NAMES, case["seqs"], [(b"last", m21)], case["rows"], **kw)
    assert stats["mirnas"] == 65537 and (tsv, summ) == want
    assert len(lines_of(tsv)) >= 3 and all(f[1] == b"last" for f in lines_of(tsv))


def test_phase_scan_after_trigger_scan(gpu_ctx, tmp_path):
    """Nothing resident changes, and the shared unit code serves both scans."""
    case = make_case(4, 22, 7, 30)
    gpu_ctx.load_genome([(n, np.full(10, 65, np.uint8)) for n in NAMES])
    gpu_ctx.load_alignments(case["alns"])
    hg = phasing.Hypergeom(7, 22)
    before, st0 = gpu_ctx.phase_scan(22, 7, hg.kmin(Fraction(1, 100)), min_phased=2, min_depth=2)
    kw = dict(Lp=22, m=7, alpha=Fraction(1, 100), K=2, D=2, flank=30, drift=2)
    tsv, summ, _ = _scan(gpu_ctx, tmp_path, NAMES, case["seqs"], case["mirna_fasta"], case["rows"], **kw)
    assert (tsv, summ) == restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], **kw)
    after, st1 = gpu_ctx.phase_scan(22, 7, hg.kmin(Fraction(1, 100)), min_phased=2, min_depth=2)
    assert before.tobytes() == after.tobytes() and st0 == st1 and len(before) > 5


def test_bad_arguments_are_refused(gpu_ctx, tmp_path):
    case = make_case(4, 21, 10, 100)
    gpu_ctx.load_genome([(n, np.full(10, 65, np.uint8)) for n in NAMES])
    gpu_ctx.load_alignments(case["alns"])
    (tmp_path / "m.fa").write_bytes(case["mirna_fasta"])
    _genome(tmp_path / "g.fa", NAMES, case["seqs"])
    km = phasing.Hypergeom(10, 21).kmin(Fraction(1, 1000))
    good = np.array([(0, 0, 10, 400)], capi.TRIGGER_LOCUS_DTYPE)
    for locus in ((-1, 0, 10, 400), (0, 4, 10, 400), (0, -1, 10, 400), (0, 0, 0, 400), (0, 0, 401, 400), (0, 0, 10, 3001)):
        with pytest.raises(capi.MirpError, match="bad locus 0"):
            gpu_ctx.trigger_scan(str(tmp_path / "m.fa"), [str(tmp_path / "g.fa")], np.array([locus], capi.TRIGGER_LOCUS_DTYPE), 21, 10, km)
    for kw in (dict(drift=3), dict(drift=-1), dict(max_half_score=17), dict(min_phased=0), dict(min_depth=0)):
        with pytest.raises(capi.MirpError, match="bad options"):
            gpu_ctx.trigger_scan(str(tmp_path / "m.fa"), [str(tmp_path / "g.fa")], good, 21, 10, km, **kw)
    (tmp_path / "bad.fa").write_bytes(b">a\nACGU\n")
    with pytest.raises(capi.MirpError, match="12..32"):
        gpu_ctx.trigger_scan(str(tmp_path / "bad.fa"), [str(tmp_path / "g.fa")], good, 21, 10, km)
    trig, counts, stats = gpu_ctx.trigger_scan(str(tmp_path / "m.fa"), [str(tmp_path / "g.fa")], good[:0], 21, 10, km)
    assert len(trig) == 0 and len(counts) == 0 and stats["sites"] == 0


# ---------------------------------------------------------------------------------------------------- the command line
def _cli(module, args, cwd, timeout=600):
    return subprocess.run([sys.executable, "-m", module] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def _phas(path, rows):
    with open(path, "wb") as f:
        f.write(phasing.HEADER)
        for name, a, b, x in rows:
            f.write(b"%s\t%d\t%d\t1\t%d\t16\t16\t1.000e-30\t90\t90\n" % (name.encode(), a, b, x))


def test_cli(tmp_path):
    Lp, m, alpha, K, D, flank, drift = 22, 8, Fraction(1, 10000), 4, 2, 40, 1
    case = make_case(11, Lp, m, flank)
    paths = [str(tmp_path / ("s%d.sam" % i)) for i in range(2)]
    write_sams(paths, NAMES, LENS, case["alns"])
    (tmp_path / "m.fa").write_bytes(case["mirna_fasta"])
    _genome(tmp_path / "g.fa", NAMES[::-1], case["seqs"][::-1])
    _phas(tmp_path / "x.phas.tsv", case["rows"])
    args = ["-l", "22", "-c", "8", "-p", "1e-4", "-k", "4", "-d", "2", "--flank", "40", "-w", "1", "m.fa", "g.fa", "x.phas.tsv"] + paths
    for p in triggers.output_names(str(tmp_path / "x.phas")):
        open(p, "wb").write(b"stale\n")
    r = _cli("mir_prefer_amd.triggers", args, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], Lp=Lp, m=m, alpha=alpha, K=K, D=D, flank=flank, drift=drift)
    assert (tmp_path / "x.phas.triggers.tsv").read_bytes() == want[0] and (tmp_path / "x.phas.triggers.summary.tsv").read_bytes() == want[1]
    assert want[0].count(b"\n") > 9
    err = r.stderr.decode().splitlines()
    assert len(err) == 1 and err[0].startswith("triggers: 11 miRNAs, %d loci, " % len(case["rows"]))
    assert err[0].endswith(" %d trigger lines written to x.phas.triggers.tsv" % (want[0].count(b"\n") - 1))
    # -o, -s and the defaults
    os.mkdir(tmp_path / "out")
    r = _cli("mir_prefer_amd.triggers", ["-l", "22", "-o", "out/y", "-s", "0", "m.fa", "g.fa", "x.phas.tsv"] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    want = restate_numpy(case["alns"], NAMES, case["seqs"], case["mirnas"], case["rows"], Lp=22, max_half=0)
    assert (tmp_path / "out" / "y.triggers.tsv").read_bytes() == want[0] and (tmp_path / "out" / "y.triggers.summary.tsv").read_bytes() == want[1]
    # a header-only phas.tsv, and no record of length Lp: headers only, exit 0
    _phas(tmp_path / "e.tsv", [])
    r = _cli("mir_prefer_amd.triggers", ["m.fa", "g.fa", "e.tsv"] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "e.triggers.tsv").read_bytes() == HEADER and (tmp_path / "e.triggers.summary.tsv").read_bytes() == SUMMARY_HEADER
    r = _cli("mir_prefer_amd.triggers", ["-l", "30", "-o", "n", "m.fa", "g.fa", "x.phas.tsv"] + paths, tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "n.triggers.tsv").read_bytes() == HEADER
    s = lines_of((tmp_path / "n.triggers.summary.tsv").read_bytes())
    assert len(s) == len(case["rows"]) and all(f[2:] == [b"0", b".", b".", b".", b"."] for f in s)
    # refusals after the device is open: a genome that lacks a contig of the SAM header, or holds it with another length
    _genome(tmp_path / "short.fa", NAMES, [s[:-1] if n == "chrA" else s for n, s in zip(NAMES, case["seqs"])])
    _genome(tmp_path / "missing.fa", NAMES[:1] + NAMES[2:], case["seqs"][:1] + case["seqs"][2:])
    _phas(tmp_path / "b.tsv", [r for r in case["rows"] if r[0] == "chrB"])
    for g, why in (("short.fa", "contig chrA has 4999 bases"), ("missing.fa", "contig short of the SAM header is not in")):
        for p in triggers.output_names(str(tmp_path / "b")):
            open(p, "wb").write(b"stale\n")
        r = _cli("mir_prefer_amd.triggers", ["m.fa", g, "b.tsv"] + paths, tmp_path)
        assert r.returncode == 255 and r.stderr.decode().startswith("Error: ") and why in r.stderr.decode(), r.stderr.decode()
        assert not any(os.path.exists(p) for p in triggers.output_names(str(tmp_path / "b")))


def test_chain_collapse_align_phasing_triggers(tmp_path):
    """The planted genome of the phasing chain test: the miRNA whose cut falls on the locus's third register boundary comes out as best_miRNA."""
    rng = np.random.RandomState(12)
    L, x0 = 21, 10001
    genome = bytearray(ACGT[rng.randint(0, 4, 30000)].tobytes())
    mirna = bytes(ACGT[rng.randint(0, 4, 21)].tobytes())
    decoy = bytes(ACGT[rng.randint(0, 4, 21)].tobytes())
    s1 = x0 + 2 * L - 11                                               # site start (1-based): the cut falls on x0 + 2L
    genome[s1 - 1:s1 - 1 + 21] = _revcomp(mirna)
    genome[x0 + 5 * L + 4:x0 + 5 * L + 25] = _revcomp(decoy)           # a perfect site off the register
    other = ACGT[rng.randint(0, 4, 5000)].tobytes()
    _genome(tmp_path / "genome.fa", ["chr1", "chr2"], [bytes(genome), other])
    reads = []
    for j in range(10):
        c = x0 + j * L
        reads += [bytes(genome[c - 1:c - 1 + L])] * 3 + [_revcomp(bytes(genome[c - 3:c - 3 + L]))] * 2
    (tmp_path / "reads.fa").write_bytes(b"".join(b">q%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    (tmp_path / "names.txt").write_text("S1\n")
    (tmp_path / "mir.fa").write_bytes(b">decoy\n" + decoy + b"\n>mir-t\n" + mirna.replace(b"T", b"U") + b"\n")
    sam = "reads.fa.processed.sam"
    for module, args in (("mir_prefer_amd.reads", ["collapse", "names.txt", "reads.fa"]),
                         ("mir_prefer_amd.align", ["-f", "-r", "genome.fa", "reads.fa.processed"]),
                         ("mir_prefer_amd.phasing", ["-g", "genome.fa", sam]),
                         ("mir_prefer_amd.triggers", ["-s", "0", "mir.fa", "genome.fa", sam + ".phas.tsv", sam])):
        r = _cli(module, args, tmp_path)
        assert r.returncode == 0, (module, r.stderr.decode())
    loci = lines_of((tmp_path / (sam + ".phas.tsv")).read_bytes())
    assert len(loci) == 1
    locus = b"chr1:%s-%s" % (loci[0][1], loci[0][2])
    cut = x0 + 2 * L
    f = lines_of((tmp_path / (sam + ".phas.triggers.tsv")).read_bytes())
    head = [locus, b"mir-t", b"chr1", b"%d" % s1, b"%d" % (s1 + 20), b"+", b"0.0", b"0", b"0", b"21", b"%d" % cut]
    # the two cycles 5' of the cut are in its register as well: the `up` window passes with 4 of 4 units
    assert [x[:13] for x in f] == [head + [b"down", b"0"], head + [b"up", b"0"]]
    assert f[0][13:15] == [b"16", b"16"] and f[0][16:19] == [b"40", b"40", b"1"] and f[1][13:15] == [b"4", b"4"] and f[1][16:19] == [b"10", b"10", b"1"]
    s = lines_of((tmp_path / (sam + ".phas.triggers.summary.tsv")).read_bytes())
    assert s == [[locus, b"2", b"2", b"mir-t", b"down", b"0", f[0][15]]]

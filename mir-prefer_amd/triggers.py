"""miRNA triggers of phased siRNA (PHAS) loci: which miRNA target site sets the phase of a locus, decided by the reads, on the GPU.

    python -m mir_prefer_amd.triggers [options] <mirna.fa> <genome.fa> <phas.tsv> <sam> [<sam2> ...]

<phas.tsv> is the output of `phasing` on the same SAM files.  Every target site of a miRNA (the score of `targets`, both strands, no mismatch at
miRNA position 10 or 11) inside a locus or its flanks sets a cut; the phasing test of `phasing` is run in the windows that the cut anchors, 3' of
it (`down`, the one-hit model) and 5' of it (`up`, the 3' site of the two-hit model), and a window that passes is a trigger line.  The SAM files
are ingested on the device and stay resident; sites and windows are found there (mirp_trigger_scan, trigger_kernels.hip).  This module turns
alpha into the exact integer kmin table, maps the contigs, writes <base>.triggers.tsv and <base>.triggers.summary.tsv and picks the best trigger
of every locus.  DESIGN.md §29 defines it all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused file and "no usable GPU" print `Error: ...`
and exit with status 255; a refused run leaves no output file, not even one from an earlier run."""
import os
import re
import sys
from optparse import OptionParser

from . import phasing
from .targets import parse_half_score

HELP = """python -m mir_prefer_amd.triggers [options] <mirna.fa> <genome.fa> <phas.tsv> <sam> [<sam2> ...]

    Find the miRNA triggers of phased siRNA (PHAS) loci on the GPU.

    <phas.tsv> is what mir_prefer_amd.phasing wrote for the same SAM files; -l must be the
    length it was run with. A miRNA target site (the score of mir_prefer_amd.targets, both
    strands, no mismatch at miRNA position 10 or 11) inside a locus or within --flank of it
    sets a cut between the target bases paired with miRNA positions 10 and 11. The phasing
    test runs in the window of -c cycles 3' of the cut (down) and in the one 5' of it (up),
    in the register the cut sets, shifted by up to -w; a window that passes is a trigger.

    Example:
    python -m mir_prefer_amd.triggers -l 21 mature.fa genome.fa sample1.sam.phas.tsv sample1.sam sample2.sam
"""

HEADER = (b"locus\tmiRNA\tcontig\tstart\tend\tstrand\tscore\tmismatches\tgu\tmirna_len\tcut\tside\toffset\tn\tk\tpvalue\tphased_reads\twindow_reads\t"
          b"locus_register\tmirna_5to3\tpairs\ttarget_3to5\n")
SUMMARY_HEADER = b"locus\tsites\ttrigger_lines\tbest_miRNA\tbest_side\tbest_offset\tbest_pvalue\n"
SIDES = (b"down", b"up")
WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"
RNA = b"ACGUN"
PAIR = b"|ox"


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.triggers")
    parser.add_option("-l", "--length", type=int, default=21, help="Phase length in nt, 18..30: the -l of the phasing run. Default 21.")
    parser.add_option("-c", "--cycles", type=int, default=10, help="Cycles per window, 4..20. Default 10.")
    parser.add_option("-p", "--pvalue", default="0.001", help="Largest p-value of a trigger window, a decimal in (0, 1] such as 0.001 or 1e-5. "
                                                              "Default 0.001.")
    parser.add_option("-k", "--min-phased", type=int, default=3, help="Fewest phased units in a trigger window, 1..2 x cycles. Default 3.")
    parser.add_option("-d", "--min-depth", type=int, default=1, help="Fewest reads of a unit; units with fewer are dropped first. Default 1.")
    parser.add_option("-s", "--max-score", default="4", help="Highest score of a site, a multiple of 0.5 in 0..8. Default 4.")
    parser.add_option("--flank", type=int, default=100, help="Bases on either side of a locus in which a site may lie, 0..2000. Default 100.")
    parser.add_option("-w", "--drift", type=int, default=0, help="Register offsets -W..W tried around the cut's register, 0..2. Default 0.")
    parser.add_option("-o", "--output", help="Output base. Default <phas.tsv> without a trailing .tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_base(phas_path):
    return phas_path[:-4] if phas_path.endswith(".tsv") else phas_path


def output_names(base):
    return [base + ".triggers.tsv", base + ".triggers.summary.tsv"]


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, mirna file, genome file, phas.tsv, SAM files, alpha, max
    half-score, output base)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 4:
        parser.error("incorrect number of arguments: a miRNA FASTA, a genome FASTA, a phas.tsv and at least one SAM file. Run with -h to see the help.")
    if not 18 <= options.length <= 30:
        parser.error("Option -l must be between 18 and 30.")
    if not 4 <= options.cycles <= 20:
        parser.error("Option -c must be between 4 and 20.")
    alpha = phasing.parse_alpha(options.pvalue)
    if alpha is None:
        parser.error("Option -p must be a decimal number greater than 0 and at most 1.")
    if not 1 <= options.min_phased <= 2 * options.cycles:
        parser.error("Option -k must be between 1 and 2 x the cycles (-c).")
    if not 1 <= options.min_depth <= phasing.MAX_DEPTH:
        parser.error("Option -d must be between 1 and %d." % phasing.MAX_DEPTH)
    half = parse_half_score(options.max_score)
    if half is None:
        parser.error("Option -s must be a multiple of 0.5 between 0 and 8.")
    if not 0 <= options.flank <= 2000:
        parser.error("Option --flank must be between 0 and 2000.")
    if not 0 <= options.drift <= 2:
        parser.error("Option -w must be between 0 and 2.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    return options, args[0], args[1], args[2], args[3:], alpha, half, options.output or output_base(args[2])


# ---------------------------------------------------------------------------------------------------- inputs
def parse_phas(data, path="phas.tsv"):
    """The bytes of a phasing output -> [(contig, start, end, best_start)] in file order; ValueError names the 1-based line."""
    if not data.startswith(phasing.HEADER):
        raise ValueError("%s: line 1: not the header line of a phasing output" % path)
    lines = data[len(phasing.HEADER):].split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out = []
    for i, ln in enumerate(lines):
        f = ln.split(b"\t")
        ok = len(f) == 10 and len(f[0]) > 0 and all(re.fullmatch(rb"-?[0-9]+", f[j]) for j in (1, 2, 3, 4, 5, 6, 8, 9))
        if not ok:
            raise ValueError("%s: line %d: not a line of a phasing output (10 tab-separated fields)" % (path, i + 2))
        try:
            name = f[0].decode()
        except UnicodeDecodeError:
            raise ValueError("%s: line %d: the contig name is not text" % (path, i + 2))
        out.append((name, int(f[1]), int(f[2]), int(f[4])))
    return out


def check_loci(rows, contig_lens, path="phas.tsv"):
    """Every locus lies on a known contig with 1 <= start <= end <= LN; ValueError names the 1-based line.  contig_lens: name -> LN."""
    for i, (name, start, end, _) in enumerate(rows):
        ln = contig_lens.get(name)
        if ln is None:
            raise ValueError("%s: line %d: unknown contig %s" % (path, i + 2, name))
        if start < 1 or start > end or end > ln:
            raise ValueError("%s: line %d: the locus %d-%d does not lie in 1..%d of contig %s" % (path, i + 2, start, end, ln, name))


def parse_mirnas(data):
    """The miRNA FASTA of DESIGN.md §14, which mirp_trigger_scan has accepted: -> [(name bytes, codes)] with A C G U/T in either case = 0..3 and
    any other letter 4; text before the first header is ignored, a tab in a name shows as a blank."""
    code = [4] * 256
    for i, ch in enumerate(b"ACGU"):
        code[ch] = code[ch + 32] = i
    code[ord("T")] = code[ord("t")] = 3
    out = []
    for line in re.split(rb"\r\n|\r|\n", data):
        if line.startswith(b">"):
            out.append((line[1:].strip(WS).replace(b"\t", b" "), []))
        elif out:
            out[-1][1].extend(code[c] for c in line.strip(WS))
    return out


_DNA = [4] * 256
for _i, _ch in enumerate(b"ACGT"):
    _DNA[_ch] = _DNA[_ch + 32] = _i


def site_columns(mc, window, strand):
    """mismatches, gu, mirna_5to3, pairs, target_3to5 of the site of the miRNA codes mc on the forward bases `window` (len(mc) of them): column i
    holds miRNA position i over the target-strand base that pairs with it (§14)."""
    L = len(mc)
    cls, ys = [], []
    for i in range(1, L + 1):
        x = _DNA[window[i - 1] if strand else window[L - i]]
        y = 3 - x if strand else x
        m = mc[i - 1]
        cls.append(0 if m < 4 and m + y == 3 else 1 if (m, y) in ((2, 3), (3, 2)) else 2)
        ys.append(y)
    return cls.count(2), cls.count(1), bytes(RNA[c] for c in mc), bytes(PAIR[c] for c in cls), bytes(RNA[y] for y in ys)


# ---------------------------------------------------------------------------------------------------- the files
def format_outputs(rows, mirnas, seqs, trig, site_counts, Lp, hg):
    """rows: parse_phas's loci; mirnas: parse_mirnas's; seqs: contig name -> bytes or uint8 array; trig: TRIGGER_DTYPE in output order; site_counts per locus.
    -> (the bytes of .triggers.tsv, the bytes of .triggers.summary.tsv)."""
    out = [HEADER]
    lines = [0] * len(rows)
    best = [None] * len(rows)
    for t in trig.tolist():
        q, m, half, strand, side, delta, n, k, o, phased, reads = t
        name, start, end, best_start = rows[q]
        mname, mc = mirnas[m]
        L = len(mc)
        cut = o + 10 if strand else o + L - 9
        r = cut - Lp + 3 if strand else cut
        p = hg.p(n, k)
        nmm, ngu, m5, pairs, t3 = site_columns(mc, bytes(seqs[name][o:o + L]), strand)
        out.append(b"%s:%d-%d\t%s\t%s\t%d\t%d\t%s\t%d.%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s\t%s\n" % (
            name.encode(), start, end, mname, name.encode(), o + 1, o + L, b"-" if strand else b"+", half // 2, 5 * (half & 1), nmm, ngu, L, cut,
            SIDES[side], delta, n, k, phasing.pvalue_text(p).encode(), phased, reads, 1 if (r + delta - best_start) % Lp == 0 else 0, m5, pairs, t3))
        lines[q] += 1
        if best[q] is None or (p, half) < best[q][:2]:
            best[q] = (p, half, mname, side, delta)
    summ = [SUMMARY_HEADER]
    for q, (name, start, end, _) in enumerate(rows):
        b = best[q]
        tail = b".\t.\t.\t." if b is None else b"%s\t%s\t%d\t%s" % (b[2], SIDES[b[3]], b[4], phasing.pvalue_text(b[0]).encode())
        summ.append(b"%s:%d-%d\t%d\t%d\t%s\n" % (name.encode(), start, end, int(site_counts[q]), lines[q], tail))
    return b"".join(out), b"".join(summ)


def scan(ctx, mirna_path, genome_path, rows, sam_names, genome, Lp, m, alpha, min_phased=3, min_depth=1, max_half_score=8, flank=100, drift=0):
    """The trigger scan on ctx's resident alignments and the two files' bytes.  rows: parse_phas's loci, already checked (check_loci); sam_names:
    the contig names the records' tids index; genome: capi.read_fasta's list of genome_path.  -> (tsv, summary, stats)."""
    from . import capi
    import numpy as np
    hg = phasing.Hypergeom(m, Lp)
    index, seqs, i = {}, {}, 0
    for name, s in genome:
        if s is not None and len(s) > 0:            # the packed genome drops empty contigs
            index[name], seqs[name] = i, s
            i += 1
    tid_of = {n: t for t, n in enumerate(sam_names)}
    loci = np.zeros(len(rows), capi.TRIGGER_LOCUS_DTYPE)
    for q, (name, start, end, _) in enumerate(rows):
        loci[q] = (tid_of[name], index[name], max(1, start - flank), min(len(seqs[name]), end + flank))
    trig, counts, stats = ctx.trigger_scan(mirna_path, [genome_path], loci, Lp, m, hg.kmin(alpha), min_phased=min_phased, min_depth=min_depth,
                                           max_half_score=max_half_score, drift=drift)
    mirnas = parse_mirnas(open(mirna_path, "rb").read())
    tsv, summ = format_outputs(rows, mirnas, seqs, trig, counts, Lp, hg)
    stats["trigger_lines"] = len(trig)
    return tsv, summ, stats


# ---------------------------------------------------------------------------------------------------- command line
def _fail(msg, paths=()):
    for p in paths:
        try:
            os.remove(p)
        except OSError:
            pass
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, mirna, genome_path, phas, sams, alpha, half, base = parse_args(argv)
    outs = output_names(base)
    for name in [mirna, genome_path, phas] + sams:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    try:
        rows = parse_phas(open(phas, "rb").read(), phas)
    except (OSError, ValueError) as e:
        return _fail(str(e))
    from . import capi
    try:
        genome = capi.read_fasta(genome_path)
        check_loci(rows, {name: len(s) for name, s in genome}, phas)
    except ValueError as e:
        return _fail(str(e))
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the trigger scan runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        try:
            names, lens, _, _, _, _ = ctx.ingest_sams(sams)
        except ValueError as e:
            return _fail(str(e))
        have = {name: len(s) for name, s in genome}
        for name, ln in zip(names, lens.tolist()):
            if name not in have:
                return _fail("contig %s of the SAM header is not in %s" % (name, genome_path))
            if have[name] != ln:
                return _fail("contig %s has %d bases in %s but LN:%d in the SAM header" % (name, have[name], genome_path, ln))
        known = set(names)
        for i, r in enumerate(rows):
            if r[0] not in known:
                return _fail("%s: line %d: unknown contig %s (not in the SAM header)" % (phas, i + 2, r[0]))
        try:
            tsv, summ, stats = scan(ctx, mirna, genome_path, rows, names, genome, options.length, options.cycles, alpha, min_phased=options.min_phased,
                                    min_depth=options.min_depth, max_half_score=half, flank=options.flank, drift=options.drift)
        except (OSError, capi.MirpError) as e:
            return _fail(str(e))
    finally:
        ctx.close()
    try:
        for p, data in zip(outs, (tsv, summ)):
            with open(p, "wb") as f:
                f.write(data)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("triggers: %d miRNAs, %d loci, %d interval bases, %d sites, %d windows evaluated, %d trigger lines written to %s\n"
                     % (stats["mirnas"], len(rows), stats["interval_bases"], stats["sites"], stats["windows"], stats["trigger_lines"], outs[0]))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

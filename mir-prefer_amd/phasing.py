"""Phased siRNA (PHAS) loci: windows whose reads fall on one 21- (or 24-) nt register on both strands, found in aligned small-RNA reads on the GPU.

    python -m mir_prefer_amd.phasing [options] <sam> [<sam2> ...]

Writes one tab-separated file of loci (default <first sam>.phas.tsv) and, with -g, their forward-strand sequences as FASTA for `targets -b`.
The SAM files are ingested on the device and stay resident; the per-anchor window scan runs there (mirp_phase_scan, phasing_kernels.hip).  This
module turns alpha into the exact integer kmin table, merges the passing windows into loci and writes the files.  DESIGN.md §15 defines it all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused SAM or genome and "no usable GPU" print
`Error: ...` and exit with status 255; a refused run leaves no output file, not even one from an earlier run."""
import math
import os
import re
import sys
from fractions import Fraction
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.phasing [options] <sam> [<sam2> ...]

    Find phased siRNA (PHAS) loci in aligned small-RNA reads on the GPU.

    Reads of length -l form units (contig, strand, register coordinate: POS on the plus
    strand, POS + 2 on the minus strand). Every unit coordinate anchors a window of -c
    cycles on both strands; a window passes when at least -k of its units are in phase
    with the anchor and the hypergeometric p-value of that count is at most -p.
    Overlapping passing windows merge into loci.

    Example:
    python -m mir_prefer_amd.phasing -l 21 -g genome.fa sample1.sam sample2.sam
"""

HEADER = b"contig\tstart\tend\twindows\tbest_start\tn\tk\tpvalue\tphased_reads\twindow_reads\n"
MAX_DEPTH = (1 << 31) - 1


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.phasing")
    parser.add_option("-l", "--length", type=int, default=21, help="Phase length in nt, 18..30. Default 21.")
    parser.add_option("-c", "--cycles", type=int, default=10, help="Cycles per window, 4..20. Default 10.")
    parser.add_option("-p", "--pvalue", default="0.001", help="Largest p-value of a passing window, a decimal in (0, 1] such as 0.001 or 1e-5. "
                                                              "Default 0.001.")
    parser.add_option("-k", "--min-phased", type=int, default=3, help="Fewest phased units in a passing window, 1..2 x cycles. Default 3.")
    parser.add_option("-d", "--min-depth", type=int, default=1, help="Fewest reads of a unit; units with fewer are dropped first. Default 1.")
    parser.add_option("-o", "--output", help="Output file. Default <first sam>.phas.tsv.")
    parser.add_option("-g", "--genome", help="Genome FASTA: also write the loci's forward-strand sequences next to the output (.fa).")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_alpha(text):
    """-p as an exact Fraction in (0, 1], or None when it is not a plain decimal ("0.001", ".5", "1e-5", "2.5E-3")."""
    if re.fullmatch(r"([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?", text or "") is None:
        return None
    a = Fraction(text)
    return a if 0 < a <= 1 else None


def output_name(sam_path):
    return sam_path + ".phas.tsv"


def fasta_name(out):
    return (out[:-4] if out.endswith(".tsv") else out) + ".fa"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, SAM files, alpha, output path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if not args:
        parser.error("incorrect number of arguments: at least one SAM file. Run with -h to see the help.")
    if not 18 <= options.length <= 30:
        parser.error("Option -l must be between 18 and 30.")
    if not 4 <= options.cycles <= 20:
        parser.error("Option -c must be between 4 and 20.")
    alpha = parse_alpha(options.pvalue)
    if alpha is None:
        parser.error("Option -p must be a decimal number greater than 0 and at most 1.")
    if not 1 <= options.min_phased <= 2 * options.cycles:
        parser.error("Option -k must be between 1 and 2 x the cycles (-c).")
    if not 1 <= options.min_depth <= MAX_DEPTH:
        parser.error("Option -d must be between 1 and %d." % MAX_DEPTH)
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if options.genome == "":
        parser.error("Option -g needs a file name.")
    return options, args, alpha, options.output or output_name(args[0])


# ---------------------------------------------------------------------------------------------------- the exact test
def _binomial_row(N):
    """C(N, i) for i = 0 .. N."""
    row = [1] * (N + 1)
    for i in range(1, N + 1):
        row[i] = row[i - 1] * (N - i + 1) // i
    return row


class Hypergeom:
    """The phasing test of one (cycles m, length L): S = 2 m L slots, G = 2 m phased slots, p(n, k) = P(at least k of n units are phased)."""

    def __init__(self, m, L):
        self.S, self.G = 2 * m * L, 2 * m
        self.cg = [math.comb(self.G, j) for j in range(self.G + 1)]
        self.cr = _binomial_row(self.S - self.G)
        self.cs = _binomial_row(self.S)
        self._p = {}

    def _term(self, n, j):
        return self.cg[j] * self.cr[n - j]

    def tail(self, n, k):
        """Sum_{j >= k} C(G, j) C(S - G, n - j): p(n, k) times C(S, n)."""
        lo, hi = max(k, n - (self.S - self.G), 0), min(n, self.G)
        return sum(self._term(n, j) for j in range(lo, hi + 1))

    def p(self, n, k):
        """p(n, k) as an exact Fraction, memoised."""
        key = (n, k)
        v = self._p.get(key)
        if v is None:
            v = self._p[key] = Fraction(self.tail(n, k), self.cs[n])
        return v

    def kmin(self, alpha):
        """kmin[n], n = 0 .. S: the smallest k with p(n, k) <= alpha (G + 1 if none), compared in integers: tail * den <= num * C(S, n)."""
        num, den = alpha.numerator, alpha.denominator
        out = []
        for n in range(self.S + 1):
            jmin, jmax = max(0, n - (self.S - self.G)), min(n, self.G)
            bound, tail, k = num * self.cs[n], 0, jmax + 1          # p(n, jmax + 1) = 0 always passes
            while k > 0:
                t = tail + (self._term(n, k - 1) if k - 1 >= jmin else 0)
                if t * den > bound:
                    break
                tail, k = t, k - 1
            out.append(k)
        return out


def pvalue_text(p):
    """%.3e of the correctly rounded double of an exact Fraction."""
    return "%.3e" % (p.numerator / p.denominator)


# ---------------------------------------------------------------------------------------------------- loci
def merge_loci(windows, contig_lens, m, L, hg):
    """Passing windows (tid, start, n, k, phased_reads, window_reads), in (tid, start) order, into loci: a window spans [x, min(x + mL - 1, LN)];
    the next window of the same contig joins while its x <= the locus' end.  The best window has the smallest exact p, then the smallest x.
    -> [(tid, start, end, windows, best window tuple, p)]."""
    out = []
    cur = None
    span = m * L
    for w in windows:
        tid, x = int(w[0]), int(w[1])
        end = min(x + span - 1, int(contig_lens[tid]))
        p = hg.p(int(w[2]), int(w[3]))
        if cur is not None and cur[0] == tid and x <= cur[2]:
            cur[2] = max(cur[2], end)
            cur[3] += 1
            if p < cur[5]:
                cur[4], cur[5] = w, p
            continue
        if cur is not None:
            out.append(tuple(cur))
        cur = [tid, x, end, 1, w, p]
    if cur is not None:
        out.append(tuple(cur))
    return out


def format_tsv(contig_names, loci):
    lines = [HEADER]
    for tid, start, end, nwin, w, p in loci:
        lines.append(("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\n" % (contig_names[tid], start, end, nwin, int(w[1]), int(w[2]), int(w[3]), pvalue_text(p),
                                                                   int(w[4]), int(w[5]))).encode())
    return b"".join(lines)


def format_fasta(contig_names, loci, seqs):
    """seqs[tid]: the contig's bytes (uint8 array or bytes)."""
    out = []
    for tid, start, end, _, _, _ in loci:
        out.append(b">%s:%d-%d\n%s\n" % (contig_names[tid].encode(), start, end, bytes(seqs[tid][start - 1:end])))
    return b"".join(out)


def window_tuples(arr):
    """A PHASE_WINDOW_DTYPE array as (tid, start, n, k, phased_reads, window_reads) tuples."""
    return list(zip(arr["tid"].tolist(), arr["start"].tolist(), arr["n"].tolist(), arr["k"].tolist(), arr["phased_reads"].tolist(),
                    arr["window_reads"].tolist()))


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
    options, sams, alpha, out = parse_args(argv)
    outs = [out] + ([fasta_name(out)] if options.genome else [])
    for name in sams + ([options.genome] if options.genome else []):
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    from . import early
    early.start_context(options.device)     # the device opens and the SAM files are tokenized while numpy imports (early.py)
    early.start_ingest(sams)
    if options.genome:
        early.start_fasta(options.genome)
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("phasing runs on the GPU and none is usable (%s); there is no CPU path." % e)
    L, m = options.length, options.cycles
    hg = Hypergeom(m, L)
    try:
        try:
            if early.has_ingest(sams):
                names, lens, _, _, _, _ = ctx.ingest_tokenized(sams)
            else:
                names, lens, _, _, _, _ = ctx.ingest_sams(sams)
        except ValueError as e:
            return _fail(str(e))
        try:
            wins, stats = ctx.phase_scan(L, m, hg.kmin(alpha), min_phased=options.min_phased, min_depth=options.min_depth)
        except capi.MirpError as e:
            return _fail(str(e))
    finally:
        ctx.close()
    loci = merge_loci(window_tuples(wins), lens, m, L, hg)
    fasta = None
    if options.genome:
        try:
            genome = dict(capi.read_fasta(options.genome))
        except ValueError as e:
            return _fail(str(e))
        seqs = []
        for name, ln in zip(names, lens.tolist()):
            s = genome.get(name)
            if s is None:
                return _fail("contig %s of the SAM header is not in %s" % (name, options.genome))
            if len(s) != ln:
                return _fail("contig %s has %d bases in %s but LN:%d in the SAM header" % (name, len(s), options.genome, ln))
            seqs.append(s)
        fasta = format_fasta(names, loci, seqs)
    try:
        with open(out, "wb") as f:
            f.write(format_tsv(names, loci))
        if fasta is not None:
            with open(outs[1], "wb") as f:
                f.write(fasta)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("phasing: %d records of length %d, %d units, %d anchors, %d passing windows, %d loci written to %s\n"
                     % (stats["records"], L, stats["units"], stats["anchors"], len(wins), len(loci), out))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

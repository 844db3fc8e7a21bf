"""Natural antisense transcripts: pairs of transcripts that can pair over a long stretch, the source of nat-siRNAs, found on the GPU.

    python -m mir_prefer_amd.nats [options] <transcripts.fa> [<more.fa> ...]

Every pair of transcripts a < b is searched by seed, join and banded extension (mirp_nats_scan, nats_kernels.hip): exact k-mers shared by a and
the reverse complement of b are binned by diagonal, and the band around every bin is aligned locally with linear gaps, Watson-Crick pairs only.
Writes <base>.tsv (one line per region), <base>.pairs.tsv (one line per pair of transcripts) and <base>.bed (two lines per region: input for
`loci --format bed` and `signature` on libraries aligned to the transcripts); <base> is <transcripts.fa>.nats unless -o names it.  DESIGN.md §36
defines the seeds, the candidates, the alignment, the selection and the files.  The host only formats what the device returns; there is no CPU
path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves none of the three files, not even one from an earlier run.  A run that finds no region
is no error: its files hold their headers only."""
import os
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.nats [options] <transcripts.fa> [<more.fa> ...]

    Find natural antisense transcripts on the GPU: the regions over which two transcripts of
    the input are complementary (A.T and C.G pairs, linear gaps), found from shared exact seeds.
    Any letter but A C G T/U equals nothing.

    Example:
    python -m mir_prefer_amd.nats -k 16 -s 200 -l 100 transcripts.fa
"""
TSV_HEADER = "name\ta\tb\tscore\ta_start\ta_end\ta_len\tb_start\tb_end\tb_len\tmatches\tmismatches\tgaps\tidentity\tseeds\tcigar\n"
PAIRS_HEADER = "a\tb\tregions\tcolumns\ta_covered\ta_cov\tb_covered\tb_cov\n"
BANDS = (16, 32, 64, 128, 256)
MAX_LEN = 65535          # MIRP_NATS_MAX_LEN: a longer transcript is skipped


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.nats")
    parser.add_option("-k", "--seed", type=int, default=16, help="Length of the exact seeds, 12..24. Default 16.")
    parser.add_option("--band", type=int, default=64, help="Diagonals per bin, one of 16 32 64 128 256; a band is three bins wide. Default 64.")
    parser.add_option("--max-occ", type=int, default=200, help="A k-mer that occurs more often, in either sense, seeds nothing, 1..10000. Default 200.")
    parser.add_option("--min-seeds", type=int, default=1, help="Smallest number of seed hits of a bin that is extended. Default 1.")
    parser.add_option("-s", "--min-score", type=int, default=200, help="Smallest score of a region, at least 1. Default 200.")
    parser.add_option("-l", "--min-length", type=int, default=100, help="Smallest number of alignment columns of a region, at least 1. Default 100.")
    parser.add_option("--match", type=int, default=3, help="Score of a pair, 1..10. Default 3.")
    parser.add_option("--mismatch", type=int, default=4, help="Penalty of two opposite bases that do not pair, 1..10. Default 4.")
    parser.add_option("--gap", type=int, default=12, help="Penalty of every base without an opposite base, 1..50. Default 12.")
    parser.add_option("-o", "--output", help="Base name of the three files. Default <transcripts.fa>.nats.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, FASTA files, base name)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 1:
        parser.error("incorrect number of arguments: at least one FASTA file. Run with -h to see the help.")
    for name, value, lo, hi in (("-k", options.seed, 12, 24), ("--max-occ", options.max_occ, 1, 10000), ("--match", options.match, 1, 10),
                                ("--mismatch", options.mismatch, 1, 10), ("--gap", options.gap, 1, 50)):
        if not lo <= value <= hi:
            parser.error("Option %s must be between %d and %d." % (name, lo, hi))
    if options.band not in BANDS:
        parser.error("Option --band must be one of %s." % " ".join(str(b) for b in BANDS))
    for name, value in (("--min-seeds", options.min_seeds), ("-s", options.min_score), ("-l", options.min_length)):
        if value < 1:
            parser.error("Option %s must be at least 1." % name)
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a base name.")
    return options, args, options.output or args[0] + ".nats"


def output_names(base):
    return base + ".tsv", base + ".pairs.tsv", base + ".bed"


def _columns(rec):
    return int(rec["matches"]) + int(rec["mismatches"]) + int(rec["gaps"])


def tsv_table(names, recs, cigars):
    """<base>.tsv: the header and one line per region, NAT_1 .. NAT_n in the records' order."""
    lines = [TSV_HEADER]
    for k, (rec, cg) in enumerate(zip(recs, cigars)):
        lines.append("NAT_%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%d\t%s\n" % (
            k + 1, names[int(rec["a"])], names[int(rec["b"])], int(rec["score"]), int(rec["a_start"]), int(rec["a_end"]), int(rec["a_len"]),
            int(rec["b_start"]), int(rec["b_end"]), int(rec["b_len"]), int(rec["matches"]), int(rec["mismatches"]), int(rec["gaps"]),
            100 * int(rec["matches"]) / _columns(rec), int(rec["seeds"]), cg))
    return "".join(lines)


def _covered(intervals):
    """Positions in the union of inclusive intervals."""
    total, reach = 0, 0
    for s, e in sorted(intervals):
        if e > reach:
            total += e - max(s - 1, reach)
            reach = e
    return total


def pairs_table(names, recs):
    """<base>.pairs.tsv: the header and one line per pair of transcripts, in the records' (a, b) order."""
    lines = [PAIRS_HEADER]
    k = 0
    while k < len(recs):
        e = k
        while e < len(recs) and (int(recs[e]["a"]), int(recs[e]["b"])) == (int(recs[k]["a"]), int(recs[k]["b"])):
            e += 1
        group = recs[k:e]
        a_cov = _covered([(int(r["a_start"]), int(r["a_end"])) for r in group])
        b_cov = _covered([(int(r["b_start"]), int(r["b_end"])) for r in group])
        lines.append("%s\t%s\t%d\t%d\t%d\t%.2f\t%d\t%.2f\n" % (
            names[int(recs[k]["a"])], names[int(recs[k]["b"])], e - k, sum(_columns(r) for r in group), a_cov, 100 * a_cov / int(recs[k]["a_len"]),
            b_cov, 100 * b_cov / int(recs[k]["b_len"])))
        k = e
    return "".join(lines)


def bed_table(names, recs):
    """<base>.bed: the interval of a, then the interval of b, of every region, named NAT_k_a and NAT_k_b (loci refuses a name that occurs twice)."""
    lines = []
    for k, rec in enumerate(recs):
        for side, t, s, e in (("a", rec["a"], rec["a_start"], rec["a_end"]), ("b", rec["b"], rec["b_start"], rec["b_end"])):
            lines.append("%s\t%d\t%d\tNAT_%d_%s\t%d\t+\n" % (names[int(t)], int(s) - 1, int(e), k + 1, side, int(rec["score"])))
    return "".join(lines)


def summary(stats, outs):
    return ("nats: %d transcripts, %d skipped, %d bases, %d k-mer values ignored, %d seed hits, %d candidates, %d kept, %d cells, %d at or above the "
            "score, %d traced, %d regions, %d pairs; written to %s, %s and %s\n" % (
                (stats["transcripts"], stats["skipped"], stats["bases"], stats["kmers_ignored"], stats["seed_hits"], stats["candidates"],
                 stats["kept_candidates"], stats["cells"], stats["above"], stats["traced"], stats["regions"], stats["pairs"]) + tuple(outs)))


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def _remove(paths):
    for p in paths:
        try:
            if os.path.lexists(p):
                os.remove(p)
        except OSError:
            pass


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, files, base = parse_args(argv)
    outs = output_names(base)
    try:
        for path in outs:
            if os.path.lexists(path):
                os.remove(path)             # outputs of an earlier run: a refused run must be left without them
    except OSError as e:
        return _fail(str(e))
    for name in files:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    from . import capi
    names, seqs, seen = [], [], set()
    for path in files:
        try:
            records = capi.read_fasta(path)
        except ValueError as e:
            return _fail("%s: %s" % (path, e))
        for k, (name, seq) in enumerate(records):
            if name in seen:
                return _fail("%s: record %d: the sequence name %s occurs twice" % (path, k + 1, name))
            if len(seq) and int(seq.max()) >= 0x80:
                return _fail("%s: record %d (%s): a byte >= 0x80" % (path, k + 1, name))
            seen.add(name)
            names.append(name)
            seqs.append(seq.tobytes())
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the search runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        recs, cigars = ctx.nats_scan(seqs, seed=options.seed, band=options.band, max_occ=options.max_occ, min_seeds=options.min_seeds,
                                     match=options.match, mismatch=options.mismatch, gap=options.gap, min_score=options.min_score,
                                     min_length=options.min_length)
        stats = ctx.nats_last_stats()
        texts = (tsv_table(names, recs, cigars), pairs_table(names, recs), bed_table(names, recs))
        for path, text in zip(outs, texts):
            with open(path, "w", encoding="latin-1", newline="") as f:
                f.write(text)
    except (OSError, capi.MirpError) as e:
        _remove(outs)
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write(summary(stats, outs))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

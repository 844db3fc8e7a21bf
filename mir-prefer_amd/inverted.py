"""Inverted repeats: where a genome can fold back on itself (hairpin-RNA loci, IR-derived siRNA loci, MITEs), found ab initio on the GPU.

    python -m mir_prefer_amd.inverted [options] <genome.fa> [<genome2.fa> ...]

Every contig is aligned with its own reverse complement inside a band of --max-span bases (a local alignment with linear gaps, the scheme of
EMBOSS einverted; mirp_inverted_scan, inverted_kernels.hip).  Writes <base>.tsv (one line per repeat), <base>.gff3 (usable as the pipeline's
GFF_FILE_INCLUDE / GFF_FILE_EXCLUDE) and <base>.fa (the repeats' sequences, input for ensemble, randfold and hairpins); <base> is
<genome.fa>.inverted unless -o names it.  DESIGN.md §30 defines the alignment, the candidate rule, the selection and the files.  The host only
formats what the device returns; there is no CPU path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves none of the three files, not even one from an earlier run.  A run that finds no repeat
is no error: its files hold their headers only."""
import os
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.inverted [options] <genome.fa> [<genome2.fa> ...]

    Find inverted repeats in a genome on the GPU: the best local alignments of every contig with
    its own reverse complement (A.T and C.G pairs, linear gaps) whose two arms lie within
    --max-span bases. Any letter but A C G T/U pairs with nothing.

    Example:
    python -m mir_prefer_amd.inverted -d 2000 -s 50 genome.fa
"""
TSV_HEADER = ("name\tcontig\tstart\tend\tscore\tleft_start\tleft_end\tright_start\tright_end\tloop\tmatches\tmismatches\tgaps\tidentity\t"
              "structure\n")
GFF_HEADER = "##gff-version 3\n"


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.inverted")
    parser.add_option("-d", "--max-span", type=int, default=2000, help="Largest extent of a repeat, both arms and the loop, 8..4096. Default 2000.")
    parser.add_option("-s", "--min-score", type=int, default=50, help="Smallest score of a repeat, at least 1. Default 50.")
    parser.add_option("--match", type=int, default=3, help="Score of a pair, 1..10. Default 3.")
    parser.add_option("--mismatch", type=int, default=4, help="Penalty of two opposite bases that do not pair, 1..10. Default 4.")
    parser.add_option("--gap", type=int, default=12, help="Penalty of every base without an opposite base, 1..50. Default 12.")
    parser.add_option("-o", "--output", help="Base name of the three files. Default <genome.fa>.inverted.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, genome files, base name)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 1:
        parser.error("incorrect number of arguments: at least one FASTA file. Run with -h to see the help.")
    for name, value, lo, hi in (("-d", options.max_span, 8, 4096), ("--match", options.match, 1, 10), ("--mismatch", options.mismatch, 1, 10),
                                ("--gap", options.gap, 1, 50)):
        if not lo <= value <= hi:
            parser.error("Option %s must be between %d and %d." % (name, lo, hi))
    if options.min_score < 1:
        parser.error("Option -s must be at least 1.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a base name.")
    return options, args, options.output or args[0] + ".inverted"


def output_names(base):
    return base + ".tsv", base + ".gff3", base + ".fa"


def _loop(rec):
    return int(rec["right_start"]) - int(rec["left_end"]) - 1


def _identity(rec):
    m, x, g = int(rec["matches"]), int(rec["mismatches"]), int(rec["gaps"])
    return 100 * m / (m + x + g)


def tsv_table(names, recs, structures):
    """<base>.tsv: the header and one line per repeat, IR_1 .. IR_n in the records' order."""
    lines = [TSV_HEADER]
    for k, (rec, st) in enumerate(zip(recs, structures)):
        lines.append("IR_%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%s\n" % (
            k + 1, names[int(rec["contig"])], int(rec["left_start"]), int(rec["right_end"]), int(rec["score"]), int(rec["left_start"]),
            int(rec["left_end"]), int(rec["right_start"]), int(rec["right_end"]), _loop(rec), int(rec["matches"]), int(rec["mismatches"]),
            int(rec["gaps"]), _identity(rec), st))
    return "".join(lines)


def gff_table(names, recs):
    """<base>.gff3: one inverted_repeat feature per repeat; no blank in the attributes, gffmask splits its lines on white space."""
    lines = [GFF_HEADER]
    for k, rec in enumerate(recs):
        lines.append("%s\tmir_prefer_amd\tinverted_repeat\t%d\t%d\t%d\t.\t.\tID=IR_%d;Left=%d..%d;Right=%d..%d;Loop=%d;Identity=%.2f\n" % (
            names[int(rec["contig"])], int(rec["left_start"]), int(rec["right_end"]), int(rec["score"]), k + 1, int(rec["left_start"]),
            int(rec["left_end"]), int(rec["right_start"]), int(rec["right_end"]), _loop(rec), _identity(rec)))
    return "".join(lines)


def fasta_table(names, contigs, recs):
    """<base>.fa: the genome bytes of every repeat, upper-cased, on one line.  contigs: bytes per contig."""
    lines = []
    for k, rec in enumerate(recs):
        s, e = int(rec["left_start"]), int(rec["right_end"])
        lines.append(">IR_%d %s:%d-%d score=%d\n%s\n" % (k + 1, names[int(rec["contig"])], s, e, int(rec["score"]),
                                                        bytes(contigs[int(rec["contig"])][s - 1:e]).decode("latin-1").upper()))
    return "".join(lines)


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
    options, genomes, base = parse_args(argv)
    outs = output_names(base)
    try:
        for path in outs:
            if os.path.lexists(path):
                os.remove(path)             # outputs of an earlier run: a refused run must be left without them
    except OSError as e:
        return _fail(str(e))
    for name in genomes:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    from . import capi
    names, contigs, seen = [], [], set()
    for path in genomes:
        try:
            records = capi.read_fasta(path)
        except ValueError as e:
            return _fail("%s: %s" % (path, e))
        for name, seq in records:
            if name in seen:
                return _fail("%s: the sequence name %s occurs twice" % (path, name))
            seen.add(name)
            names.append(name)
            contigs.append(seq.tobytes())
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the search runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        recs, structures = ctx.inverted_scan(contigs, max_span=options.max_span, min_score=options.min_score, match=options.match,
                                             mismatch=options.mismatch, gap=options.gap)
        stats = ctx.inverted_last_stats()
        texts = (tsv_table(names, recs, structures), gff_table(names, recs), fasta_table(names, contigs, recs))
        for path, text in zip(outs, texts):
            with open(path, "w", encoding="latin-1", newline="") as f:
                f.write(text)
    except (OSError, capi.MirpError) as e:
        _remove(outs)
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write("inverted: %d contigs, %d bases, %d cells, %d rows at or above %d, %d candidates, %d traced, %d dropped untraced, %d accepted; "
                     "written to %s, %s and %s\n" % ((stats["contigs"], stats["bases"], stats["cells"], stats["rows_above"], options.min_score,
                                                      stats["candidates"], stats["traced"], stats["dropped_untraced"], stats["accepted"]) + outs))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Known-miRNA annotation: which predicted miRNAs (or collapsed reads) are known miRNAs, isomiRs or homologs of them, and which are novel, on the GPU.

    python -m mir_prefer_amd.annotate [options] <query.fa> <known.fa> [<known2.fa> ...]

Every query sequence is compared with every known sequence (a miRBase mature.fa, say) in the same sense, without gaps, at the few shifts that keep
both ends within -e nucleotides (mirp_annotate_scan, annotate_kernels.hip).  Writes one tab-separated file of hits (default <query.fa>.annot.tsv)
and one line per query to a summary file beside it.  DESIGN.md §19 defines the comparison, the order and both files.  There is no CPU path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves neither output file, not even one from an earlier run."""
import os
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.annotate [options] <query.fa> <known.fa> [<known2.fa> ...]

    Annotate miRNAs against known miRNAs (e.g. miRBase mature.fa) on the GPU.

    A query (12..32 nt, A C G U/T; any other letter mismatches) hits a known sequence when
    some ungapped, same-sense placement has at most -m mismatches and both ends within -e
    nucleotides of the known sequence's ends. Each query is classed identical, isomir
    (no mismatch, other ends), homolog (mismatches) or novel (no hit) by its best hit.

    Example:
    python -m mir_prefer_amd.annotate --species ath,osa out/prefix_miRNA.mature.fa mature.fa
"""


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.annotate")
    parser.add_option("-e", "--max-offset", type=int, default=2, help="Largest distance between the query's and the known sequence's 5' ends, and 3' ends, 0..4. Default 2.")
    parser.add_option("-m", "--max-mismatches", type=int, default=2, help="Most mismatches in the overlap, 0..6. Default 2.")
    parser.add_option("-k", "--max-hits", type=int, default=0, help="Write the first N hits per query, in output order; 0 = all (default).")
    parser.add_option("--species", help="Comma-separated id prefixes (ath,osa,...): keep only the known sequences whose id starts with one of them and '-'.")
    parser.add_option("-o", "--output", help="Hits file. Default <query.fa>.annot.tsv. The summary goes to the same name with .summary.tsv for .tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_name(query_path):
    return query_path + ".annot.tsv"


def summary_name(hits_path):
    """<hits file minus a final .tsv>.summary.tsv"""
    return (hits_path[:-4] if hits_path.endswith(".tsv") else hits_path) + ".summary.tsv"


def parse_species(text):
    """--species as a list of prefixes; None when the list or one of its entries is empty."""
    parts = text.split(",")
    return None if any(p == "" for p in parts) else parts


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, query file, known files, species list, hits path, summary path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a query FASTA and at least one FASTA of known miRNAs. Run with -h to see the help.")
    if not 0 <= options.max_offset <= 4:
        parser.error("Option -e must be between 0 and 4.")
    if not 0 <= options.max_mismatches <= 6:
        parser.error("Option -m must be between 0 and 6.")
    if options.max_hits < 0:
        parser.error("Option -k must be at least 0.")
    species = []
    if options.species is not None:
        species = parse_species(options.species)
        if species is None:
            parser.error("Option --species needs a non-empty, comma-separated list of non-empty prefixes.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    out = options.output or output_name(args[0])
    return options, args[0], args[1:], species, out, summary_name(out)


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, query, known, species, out, summary = parse_args(argv)
    for name in [query] + known:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for path in (out, summary):
            if os.path.lexists(path):
                os.remove(path)             # outputs of an earlier run: a refused run must be left without them
    except OSError as e:
        return _fail(str(e))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the annotation runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        res = ctx.annotate_scan(query, known, out, summary, max_offset=options.max_offset, max_mismatches=options.max_mismatches,
                                max_lines=options.max_hits, species=species)
    except (OSError, capi.MirpError) as e:
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write("annotate: %d queries, %d known sequences kept (%d skipped), %d pairs, %d hits; %d identical, %d isomir, %d homolog, %d novel; "
                     "written to %s and %s\n" % (res["queries"], res["known"], res["skipped"], res["pairs"], res["hits"], res["identical"], res["isomir"],
                                                 res["homolog"], res["novel"], out, summary))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Degradome (PARE / GMUCT) evidence of miRNA-guided cleavage: which predicted target sites are cut, on the GPU.

    python -m mir_prefer_amd.degradome [options] <mirna.fa> <transcripts.fa> <degradome.sam> [<degradome2.sam> ...]

The SAM files hold the degradome reads aligned to the transcripts (trim -> reads collapse -> align -r transcripts.fa); they are ingested on the
device and pooled.  The 5' ends of the sense reads are the units; every miRNA is evaluated only at the units, with its position 10 on the unit
(mirp_degradome_scan, degradome_kernels.hip).  Writes one tab-separated file of hits (default <first sam>.degradome.tsv).  DESIGN.md §18 defines
the units, their categories, the hits, the p-value and the output.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves no output file, not even one from an earlier run."""
import os
import re
import sys
from fractions import Fraction
from optparse import OptionParser

from .targets import parse_half_score

HELP = """python -m mir_prefer_amd.degradome [options] <mirna.fa> <transcripts.fa> <degradome.sam> [<degradome2.sam> ...]

    Confirm miRNA target cleavage with degradome (PARE) reads on the GPU.

    The 5' ends of the degradome reads on the plus strand of a transcript are grouped by
    position and ranked in categories 0 (the transcript's single highest peak) to 4 (one
    read). A miRNA hits a position when the site that pairs its nucleotide 10 with that
    position scores at most -s (the score of mir_prefer_amd.targets); the p-value is the
    chance that one of the miRNA's sites at that score falls on such a position by accident.

    Example:
    python -m mir_prefer_amd.degradome -s 5 -p 0.05 out/prefix_miRNA.mature.fa cdna.fa degradome.fa.processed.sam
"""

_DECIMAL = r"([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?"


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.degradome")
    parser.add_option("-s", "--max-score", default="4", help="Highest score of a hit, a multiple of 0.5 in 0..8. Default 4.")
    parser.add_option("-c", "--cleavage-site", action="store_true", help="Reject sites with a mismatch (not a G:U) at miRNA position 10 or 11.")
    parser.add_option("--max-category", type=int, default=4, help="Evaluate positions of category 0..N only, 0..4. Default 4.")
    parser.add_option("-p", "--max-pvalue", default="1", help="Highest p-value written, greater than 0 and at most 1 (0.05, 1e-3). Default 1.")
    parser.add_option("-o", "--output", help="Output file. Default <first sam>.degradome.tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_alpha(text):
    """-p as a float in (0, 1], or None."""
    if re.fullmatch(_DECIMAL, text or "") is None:
        return None
    return float(text) if 0 < Fraction(text) <= 1 else None


def output_name(sam_path):
    return sam_path + ".degradome.tsv"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, mirna file, transcript file, SAM files, max half-score, alpha,
    output path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 3:
        parser.error("incorrect number of arguments: a miRNA FASTA, a transcript FASTA and at least one SAM file. Run with -h to see the help.")
    half = parse_half_score(options.max_score)
    if half is None:
        parser.error("Option -s must be a multiple of 0.5 between 0 and 8.")
    if not 0 <= options.max_category <= 4:
        parser.error("Option --max-category must be between 0 and 4.")
    alpha = parse_alpha(options.max_pvalue)
    if alpha is None:
        parser.error("Option -p must be a number greater than 0 and at most 1.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    return options, args[0], args[1], args[2:], half, alpha, options.output or output_name(args[2])


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def summary(res, out):
    return ("degradome: %d records, %d sense records, %d units (categories 0..4: %d / %d / %d / %d / %d), %d evaluations, %d hits written to %s\n"
            % (res["records"], res["sense"], res["units"], res["c0"], res["c1"], res["c2"], res["c3"], res["c4"], res["evaluations"], res["hits"], out))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, mirna, transcripts, sams, half, alpha, out = parse_args(argv)
    for name in [mirna, transcripts] + sams:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        if os.path.lexists(out):
            os.remove(out)                  # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    from . import early
    early.start_context(options.device)     # the device opens and the SAM files are tokenized while numpy imports (early.py)
    early.start_ingest(sams)
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the degradome scan runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        try:
            if early.has_ingest(sams):
                names, lens, _, _, _, _ = ctx.ingest_tokenized(sams)
            else:
                names, lens, _, _, _, _ = ctx.ingest_sams(sams)
        except ValueError as e:
            return _fail(str(e))
        try:
            res = ctx.degradome_scan(mirna, transcripts, out, names, lens, max_half_score=half, cleavage_site=bool(options.cleavage_site),
                                     max_category=options.max_category, alpha=alpha)
        except (OSError, capi.MirpError) as e:
            return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write(summary(res, out))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Endogenous target mimics (eTMs): transcripts that pair with a miRNA around a loop of unpaired bases opposite its cleavage site, found on the GPU.

    python -m mir_prefer_amd.mimics [options] <mirna.fa> <target.fa> [<target2.fa> ...]

Writes one tab-separated file of sites (default <mirna.fa>.mimics.tsv).  The search runs in one device context (mirp_mimic_scan,
mimic_kernels.hip); there is no CPU path.  The sites and the output are defined in DESIGN.md §27.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...` and
exit with status 255; a refused run leaves no output file, not even one from an earlier run."""
import os
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.mimics [options] <mirna.fa> <target.fa> [<target2.fa> ...]

    Find endogenous target mimics of miRNAs in transcripts or a genome on the GPU.

    A mimic site pairs with the whole miRNA (12..32 nt, A C G U/T; any other letter
    mismatches) but carries a loop of -l unpaired target bases between the bases paired
    with miRNA positions P and P+1, P = 9, 10 or 11: opposite the cleavage site, so the
    target is bound and not sliced (IPS1 / miR399). Positions 2..8 must be Watson-Crick
    pairs, the two pairs that close the loop must not be mismatches (a G:U passes), and the
    mismatches and G:U pairs of the whole miRNA together (`imperfect`) are at most -n. Per
    miRNA, interval and strand the loop position with the lowest `imperfect` is written
    (column `loop`), the smallest on a tie. The three alignment columns show the loop as
    `-` under the unpaired target bases. Sites are written whether or not an ungapped
    target site overlaps them.

    Example:
    python -m mir_prefer_amd.mimics -b out/prefix_miRNA.mature.fa lncrna.fa
"""


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.mimics")
    parser.add_option("-n", "--max-imperfect", type=int, default=3, help="Most mismatches and G:U pairs together, 0..6. Default 3.")
    parser.add_option("-l", "--loop-length", type=int, default=3, help="Unpaired target bases of the loop, 2..6. Default 3.")
    parser.add_option("-b", "--both-strands", action="store_true", help="Also scan the minus strand of the targets (for genome-sized targets).")
    parser.add_option("-k", "--max-sites", type=int, default=0, help="Write the first N sites per miRNA, in output order; 0 = all (default).")
    parser.add_option("-o", "--output", help="Output file. Default <mirna.fa>.mimics.tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_name(mirna_path):
    return mirna_path + ".mimics.tsv"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, mirna file, target files, output path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a miRNA FASTA and at least one target FASTA. Run with -h to see the help.")
    if not 0 <= options.max_imperfect <= 6:
        parser.error("Option -n must be between 0 and 6.")
    if not 2 <= options.loop_length <= 6:
        parser.error("Option -l must be between 2 and 6.")
    if options.max_sites < 0:
        parser.error("Option -k must be at least 0.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    return options, args[0], args[1:], options.output or output_name(args[0])


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, mirna, targets, out = parse_args(argv)
    for name in [mirna] + targets:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        if os.path.lexists(out):
            os.remove(out)                  # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the mimic search runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        res = ctx.mimic_scan(mirna, targets, out, max_imperfect=options.max_imperfect, loop_len=options.loop_length,
                             both_strands=bool(options.both_strands), max_sites=options.max_sites)
    except (OSError, capi.MirpError) as e:
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write("mimics: %d miRNAs (%d without a usable seed), %d targets, %d bases scanned (%s), %d sites written to %s\n"
                     % (res["mirnas"], res["no_seed"], res["targets"], res["bases"], "both strands" if options.both_strands else "plus strand",
                        res["sites"], out))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

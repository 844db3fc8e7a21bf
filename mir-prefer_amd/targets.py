"""Plant miRNA target sites: every miRNA against every offset of every transcript (or genome contig), scored by position-weighted mismatches, on the GPU.

    python -m mir_prefer_amd.targets [options] <mirna.fa> <target.fa> [<target2.fa> ...]

Writes one tab-separated file of sites (default <mirna.fa>.targets.tsv).  The search runs in one device context (mirp_target_scan,
targets_kernels.hip); there is no CPU path.  The sites, their score and the output are defined in DESIGN.md §14.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...` and
exit with status 255; a refused run leaves no output file, not even one from an earlier run."""
import os
import re
import sys
from fractions import Fraction
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.targets [options] <mirna.fa> <target.fa> [<target2.fa> ...]

    Find plant miRNA target sites in transcripts on the GPU.

    Every miRNA (12..32 nt, A C G U/T; any other letter mismatches) is paired with every
    offset of every target, without gaps. A site's score sums 1 per mismatch and 0.5 per
    G:U pair, doubled at miRNA positions 2..13; sites scoring at most -s are written.
    With -g, sites with one unpaired nucleotide (a bulge on the target or on the miRNA,
    costing 1, or 2 inside positions 2..13) are written too, and every line ends with a
    column `bulge`: `.`, `tP` or `mP`, P = the miRNA position before the unpaired target
    base, or the unpaired miRNA position itself.
    With -e, every line ends with four more columns: `mfe`, the minimum free energy
    (kcal/mol, Turner 2004) of the duplex of the miRNA with the site and one flanking base
    on each side, folded freely; `mfe_perfect`, that of the miRNA with its reverse
    complement; `mfe_ratio`, mfe / mfe_perfect to three decimals (NA when mfe_perfect is
    0); and `duplex`, the structure: the miRNA as ( and ., then &, then the target strand
    5'->3' as ) and .
    With -u, every line ends with a last column `upe`: the energy (kcal/mol, three
    decimals) that opens the site inside its window of the target strand, i.e. -kT ln of
    the probability that no base of the site is paired when the window folds alone. The
    window is the site with --flank-up bases towards the 5' end of the target strand and
    --flank-down towards its 3' end, clipped to the transcript. 0.000 = already open.

    Example:
    python -m mir_prefer_amd.targets -s 3 -c out/prefix_miRNA.mature.fa cdna.fa
"""


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.targets")
    parser.add_option("-s", "--max-score", default="4", help="Highest score written, a multiple of 0.5 in 0..8. Default 4.")
    parser.add_option("-b", "--both-strands", action="store_true", help="Also scan the minus strand of the targets (for genome-sized targets).")
    parser.add_option("-c", "--cleavage-site", action="store_true", help="Reject sites with a mismatch (not a G:U) at miRNA position 10 or 11.")
    parser.add_option("-g", "--bulge", action="store_true", help="Also write sites with exactly one unpaired nucleotide; adds the column `bulge`.")
    parser.add_option("-e", "--energy", action="store_true", help="Fold every site's miRNA:target duplex; adds the columns `mfe mfe_perfect mfe_ratio duplex`.")
    parser.add_option("-u", "--accessibility", action="store_true", help="Fold every site's window of the target; adds the column `upe`.")
    parser.add_option("--flank-up", type=int, default=None, help="With -u: bases of the window 5' of the site on the target strand. Default 17.")
    parser.add_option("--flank-down", type=int, default=None, help="With -u: bases of the window 3' of the site on the target strand. Default 13.")
    parser.add_option("-k", "--max-sites", type=int, default=0, help="Write the first N sites per miRNA, in output order; 0 = all (default).")
    parser.add_option("-o", "--output", help="Output file. Default <mirna.fa>.targets.tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_half_score(text):
    """-s as half-units ("4" -> 8, "2.5" -> 5), or None when it is not a decimal multiple of 0.5 in 0..8."""
    if re.fullmatch(r"[0-9]+(\.[0-9]*)?|\.[0-9]+", text or "") is None:
        return None
    h = Fraction(text) * 2
    return int(h) if h.denominator == 1 and 0 <= h <= 16 else None


def output_name(mirna_path):
    return mirna_path + ".targets.tsv"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, mirna file, target files, max half-score, output path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a miRNA FASTA and at least one target FASTA. Run with -h to see the help.")
    half = parse_half_score(options.max_score)
    if half is None:
        parser.error("Option -s must be a multiple of 0.5 between 0 and 8.")
    if options.max_sites < 0:
        parser.error("Option -k must be at least 0.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if not options.accessibility and (options.flank_up is not None or options.flank_down is not None):
        parser.error("Options --flank-up and --flank-down need -u.")
    options.flank_up = 17 if options.flank_up is None else options.flank_up
    options.flank_down = 13 if options.flank_down is None else options.flank_down
    if options.flank_up < 0 or options.flank_down < 0 or options.flank_up + options.flank_down > 95:
        parser.error("Options --flank-up and --flank-down must be at least 0 and at most 95 together.")
    return options, args[0], args[1:], half, options.output or output_name(args[0])


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, mirna, targets, half, out = parse_args(argv)
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
        return _fail("the target search runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        res = ctx.target_scan(mirna, targets, out, max_half_score=half, both_strands=bool(options.both_strands),
                              cleavage_site=bool(options.cleavage_site), max_sites=options.max_sites, bulge=bool(options.bulge), energy=bool(options.energy),
                              accessibility=bool(options.accessibility), flanks=(options.flank_up, options.flank_down))
    except (OSError, capi.MirpError) as e:
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write("targets: %d miRNAs, %d targets, %d bases scanned (%s), %d sites written to %s\n"
                     % (res["mirnas"], res["targets"], res["bases"], "both strands" if options.both_strands else "plus strand", res["sites"], out))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

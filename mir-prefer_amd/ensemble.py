"""Partition function of precursors: ensemble free energy, frequency of the MFE structure, ensemble diversity, centroid structure and base-pair
probabilities, on the GPU.

    python -m mir_prefer_amd.ensemble [-p] [-c CUTOFF] [-o OUT] [--device N] <precursors.fa>

Every sequence of the FASTA file is folded inside / outside over all its secondary structures on the device (mirp_ensemble, ensemble_kernels.hip;
Turner 2004, dangles 2), and one record per sequence comes back.  Writes one tab-separated line per sequence (default
<precursors.fa>.ensemble.tsv): the MFE, the ensemble free energy, the frequency of the MFE structure in the ensemble, the ensemble diversity, the
centroid's distance to the ensemble and the centroid structure.  With -p the pairs with probability >= -c go to <OUT minus .tsv>.bpp.tsv as
`name i j p`, positions 1-based.  DESIGN.md §23 defines the model and every quantity.  There is no CPU path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves no output file, not even one from an earlier run."""
import os
import sys
from optparse import OptionParser

from .randfold import parse_fasta

HELP = """python -m mir_prefer_amd.ensemble [options] <precursors.fa>

    Fold every sequence (1..3000 nt; A C G U/T, any other letter folds as N) over all its
    secondary structures on the GPU: ensemble free energy, frequency of the MFE structure,
    ensemble diversity, centroid structure and, with -p, the base-pair probabilities.

    Example:
    python -m mir_prefer_amd.ensemble -p out/prefix_miRNA.precursor.fa
"""
HEADER = "name\tlength\tmfe\tefe\tmfe_freq\tdiversity\tcentroid_dist\tcentroid\n"


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.ensemble")
    parser.add_option("-p", "--pairs", action="store_true", default=False, help="Also write the base-pair probabilities (<OUT minus .tsv>.bpp.tsv).")
    parser.add_option("-c", "--cutoff", type=float, default=0.001, help="Smallest probability -p writes, in (0, 1]. Default 0.001.")
    parser.add_option("-o", "--output", help="Output file. Default <precursors.fa>.ensemble.tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_name(path):
    return path + ".ensemble.tsv"


def bpp_name(out):
    return (out[:-4] if out.endswith(".tsv") else out) + ".bpp.tsv"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, input file, output path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) != 1:
        parser.error("incorrect number of arguments: one FASTA file of precursors. Run with -h to see the help.")
    if not 0 < options.cutoff <= 1:          # (a NaN fails both comparisons)
        parser.error("Option -c must be greater than 0 and at most 1.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    return options, args[0], options.output or output_name(args[0])


def table_line(name, rec, centroid):
    """One line of the table from a record (len, mfe, efe, mfe_freq, diversity, centroid_dist) and the centroid text."""
    def f2(x):
        return "%.2f" % (0 - (0 - float(x)))          # (-0.0 prints as 0.00)
    fields = [name, "%d" % int(rec["len"]), f2(int(rec["mfe"]) / 100), f2(rec["efe"]), "%.6g" % float(rec["mfe_freq"]), f2(rec["diversity"]),
              f2(rec["centroid_dist"]), centroid]
    return "\t".join(fields) + "\n"


def table(names, recs, centroids):
    return HEADER + "".join(table_line(name, rec, cen.decode("ascii") if isinstance(cen, bytes) else cen) for name, rec, cen in zip(names, recs, centroids))


def bpp_table(names, bpp):
    return "".join("%s\t%d\t%d\t%.6f\n" % (names[int(r["seq"])], int(r["i"]), int(r["j"]), float(r["p"])) for r in bpp)


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
    options, path, out = parse_args(argv)
    outs = [out, bpp_name(out)]
    if not os.path.isfile(path):
        return _fail("file " + path + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # the outputs of an earlier run: a refused run must be left without them
        with open(path, "rb") as f:
            records = parse_fasta(f.read())
    except (OSError, ValueError) as e:
        return _fail("%s: %s" % (path, e) if isinstance(e, ValueError) else str(e))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the partition function is computed on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        recs, cens, bpp = ctx.ensemble([s for _, s in records], options.cutoff if options.pairs else None)
        stats = ctx.ensemble_last_stats()
        names = [name.decode("latin-1") for name, _ in records]
        with open(out, "w", encoding="latin-1", newline="") as f:
            f.write(table(names, recs, cens))
        if options.pairs:
            with open(outs[1], "w", encoding="latin-1", newline="") as f:
                f.write(bpp_table(names, bpp))
    except (OSError, capi.MirpError) as e:
        _remove(outs)
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write("ensemble: %d precursors, %d cells, %d passes; written to %s\n" % (stats["sequences"], stats["cells"], stats["passes"], out))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

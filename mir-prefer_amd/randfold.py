"""Shuffle test of precursor MFEs (randfold): does a precursor fold better than chance, on the GPU.

    python -m mir_prefer_amd.randfold [options] <precursors.fa>

Every sequence of the FASTA file is shuffled -n times on the device (keeping its dinucleotide counts, or only its composition with -m mono), the
sequence and its shuffles are folded there, and the MFEs come back as one integer record per sequence (mirp_randfold, randfold_kernels.hip).  Writes
one tab-separated line per sequence (default <precursors.fa>.randfold.tsv) with the MFE, AMFE and MFEI of the sequence, the share p of shuffles that
fold at least as well, and the mean, standard deviation and z-score of the shuffled MFEs.  DESIGN.md §20 defines the shuffles, the random numbers
and the table.  There is no CPU path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves no output file, not even one from an earlier run."""
import math
import os
import re
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.randfold [options] <precursors.fa>

    Score the MFE of every sequence (1..3000 nt; A C G U/T, any other letter folds as N)
    against the MFEs of its shuffles, on the GPU: p = (shuffles that fold at least as well
    + 1) / (shuffles + 1), with AMFE, MFEI and the z-score beside it.

    Example:
    python -m mir_prefer_amd.randfold -n 999 out/prefix_miRNA.precursor.fa
"""
HEADER = "name\tlength\tgc\tmfe\tamfe\tmfei\tshuffles\tle\tp\tmean\tsd\tz\n"
FOLD_MODELS = ("vienna-2.1.2", "vienna-1.8.5")


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.randfold")
    parser.add_option("-n", "--shuffles", type=int, default=999, help="Shuffles per sequence, 1..100000. Default 999.")
    parser.add_option("-m", "--method", default="di", help="mono: shuffle the letters; di: keep every dinucleotide count and both ends. Default di.")
    parser.add_option("--seed", default="0", help="Seed of the random numbers, 0..2^64-1. Default 0.")
    parser.add_option("--fold-model", dest="fold_model", default="vienna-2.1.2", choices=list(FOLD_MODELS),
                      help="Which RNALfold the fold reproduces: 2.1.2 (Turner-2004, dangles 2; default) or 1.8.5 (Turner-1999, dangles 1).")
    parser.add_option("-o", "--output", help="Output file. Default <precursors.fa>.randfold.tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_name(path):
    return path + ".randfold.tsv"


def parse_seed(text):
    """--seed as an integer 0..2^64-1 (decimal, or 0x... hexadecimal); None when it is not one."""
    try:
        v = int(text, 0)
    except ValueError:
        return None
    return v if 0 <= v < 1 << 64 else None


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, input file, seed, output path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) != 1:
        parser.error("incorrect number of arguments: one FASTA file of precursors. Run with -h to see the help.")
    if not 1 <= options.shuffles <= 100000:
        parser.error("Option -n must be between 1 and 100000.")
    if options.method not in ("mono", "di"):
        parser.error("Option -m must be mono or di.")
    seed = parse_seed(options.seed)
    if seed is None:
        parser.error("Option --seed must be an integer between 0 and 2^64-1.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    return options, args[0], seed, options.output or output_name(args[0])


def parse_fasta(data):
    """FASTA bytes -> [(name, sequence)], both bytes: the name is the first word of the header, the lines of a sequence are joined without their
    white space, text before the first header is ignored.  ValueError for a header without a name."""
    out = []
    for line in re.split(rb"\r\n|\r|\n", data):
        if line.startswith(b">"):
            words = line[1:].split()
            if not words:
                raise ValueError("record %d: a header without a name" % (len(out) + 1))
            out.append((words[0], []))
        elif out:
            out[-1][1].append(b"".join(line.split()))
    return [(name, b"".join(parts)) for name, parts in out]


def table_line(name, rec, n):
    """One line of the table from the integers of a record (len, gc, mfe, le, sum, sum_sq) and the number of shuffles."""
    length, gc, mfe, le, s, q = (int(rec[f]) for f in ("len", "gc", "mfe", "le", "sum", "sum_sq"))
    var = n * q - s * s
    spread = math.sqrt(var / (n * (n - 1))) if n > 1 else None
    fields = [name, "%d" % length, "%.2f" % (100 * gc / length), "%.2f" % (mfe / 100), "%.2f" % ((0 - mfe) / length),
              "%.4f" % ((0 - mfe) / (100 * gc)) if gc else "NA", "%d" % n, "%d" % le, "%.6f" % ((le + 1) / (n + 1)), "%.2f" % (s / n / 100),
              "%.2f" % (spread / 100) if n > 1 else "NA", "%.3f" % ((mfe - s / n) / spread) if n > 1 and var != 0 else "NA"]
    return "\t".join(fields) + "\n"


def table(names, recs, n):
    return HEADER + "".join(table_line(name, rec, n) for name, rec in zip(names, recs))


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, path, seed, out = parse_args(argv)
    if not os.path.isfile(path):
        return _fail("file " + path + " does not exist!!!")
    try:
        if os.path.lexists(out):
            os.remove(out)                  # the output of an earlier run: a refused run must be left without it
        with open(path, "rb") as f:
            records = parse_fasta(f.read())
    except (OSError, ValueError) as e:
        return _fail("%s: %s" % (path, e) if isinstance(e, ValueError) else str(e))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the shuffles are made and folded on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        ctx.set_fold_model(options.fold_model)
        recs, res = ctx.randfold([s for _, s in records], options.shuffles, options.method == "di", seed)
        text = table([name.decode("latin-1") for name, _ in records], recs, options.shuffles)
        with open(out, "w", encoding="latin-1", newline="") as f:
            f.write(text)
    except (OSError, capi.MirpError) as e:
        try:
            if os.path.lexists(out):
                os.remove(out)
        except OSError:
            pass
        return _fail(str(e))
    finally:
        ctx.close()
    sec = res["seconds"]
    sys.stderr.write("randfold: %d precursors, %d folds, %d passes, %.3f s (upload %.3f, shuffle %.3f, fold %.3f, statistics %.3f, download %.3f); "
                     "written to %s\n" % (res["sequences"], res["folds"], res["passes"], sum(sec), sec[0], sec[1], sec[2], sec[3], sec[4], out))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

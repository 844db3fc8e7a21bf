"""Profile of a raw small-RNA library before `trim`: its 3' adapter, found from the reads themselves, the insert-length distribution by 5' base
and the composition and quality per cycle, on the GPU.

    python -m mir_prefer_amd.libqc [options] <reads1> ... <readsN>

Every input X (FASTQ or FASTA, a `.gz` suffix dropped first) gives three tables next to it:

    X.libqc.tsv           key / value: reads, sampled, adapter, status, seed, seed_count, left_steps, left_stop, with_adapter, dimers, insert_mode
    X.libqc.lengths.tsv   length, raw reads, inserts, inserts by 5' base (A C G T other), up to the last length that occurs
    X.libqc.cycles.tsv    cycle, A C G T other, mean quality to three decimals, up to the last cycle that occurs

and one line on stdout with the adapter and the `trim` command that uses it.  The adapter is walked out of a table of 12-mer counts over the first
--sample reads (mirp_libqc_reads, libqc_kernels.hip); status `ok` means the walk found the adapter's start, `unsure` that the candidate may be an
abundant insert (an already trimmed file), `none` that no 12-mer is frequent enough.  The insert table uses -a when given, else the found adapter,
under `trim`'s adapter rule with -e and -O.  What is counted and how the adapter is found is defined in DESIGN.md §35; the input rules, the
refusals and the exit statuses are those of `trim`."""
import os
import re
import sys
from optparse import OptionParser

from .trim import ADAPTER_MAX, parse_permille, read_input

HELP = """python -m mir_prefer_amd.libqc [options] <reads1> ... <readsN>

    Find the 3' adapter of raw small-RNA reads and profile them on the GPU: insert lengths by
    5' base, base composition and quality per cycle.

    The input is FASTQ (Phred+33) or FASTA, plain or gzip-compressed. Every input X gives
    X.libqc.tsv, X.libqc.lengths.tsv and X.libqc.cycles.tsv (X without a .gz suffix) next to it.

    Example:
    python -m mir_prefer_amd.libqc lib1.fastq.gz lib2.fastq.gz
"""
SAMPLE_DEFAULT = 1 << 20
SAMPLE_MAX = 1 << 26
SUFFIXES = (".libqc.tsv", ".libqc.lengths.tsv", ".libqc.cycles.tsv")


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.libqc")
    parser.add_option("-a", "--adapter", help="3' adapter for the insert table, 1..64 characters of ACGT (either case). Without it, the found one.")
    parser.add_option("-e", "--error-rate", default="0.1", help="Mismatches allowed per overlap base, 0 <= E < 1, at most three decimals. Default 0.1.")
    parser.add_option("-O", "--overlap", type=int, default=None, help="Minimum overlap with the adapter, 1..64 (at most the adapter's length). Default 3.")
    parser.add_option("--sample", type=int, default=SAMPLE_DEFAULT, help="Reads, from the first on, that the adapter is found from, 1..2^26. Default 2^20.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, files, error_permille)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 1:
        parser.error("incorrect number of arguments. Run with -h to see the help.")
    adapter = options.adapter
    if adapter is not None and (not 1 <= len(adapter) <= ADAPTER_MAX or re.fullmatch(r"[ACGTacgt]+", adapter) is None):
        parser.error("Option -a must be 1..64 characters of ACGT.")
    pm = parse_permille(options.error_rate)
    if pm is None:
        parser.error("Option -e must be a decimal 0 <= E < 1 with at most three decimals.")
    if options.overlap is not None and not 1 <= options.overlap <= (len(adapter) if adapter else ADAPTER_MAX):
        parser.error("Option -O must be between 1 and the adapter length (%d)." % (len(adapter) if adapter else ADAPTER_MAX))
    if not 1 <= options.sample <= SAMPLE_MAX:
        parser.error("Option --sample must be between 1 and 2^26.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    return options, args, pm


def output_names(path):
    stem = path[:-3] if path.endswith(".gz") else path
    return tuple(stem + s for s in SUFFIXES)


def insert_mode(insert):
    """The insert length past 0 with the most reads, ties to the shortest; 0 without any."""
    best, at = 0, 0
    for length in range(1, len(insert)):
        if insert[length][5] > best:
            best, at = int(insert[length][5]), length
    return at


def render(res):
    """The three tables of one result of capi.Context.libqc_reads, as bytes."""
    summary = ["reads\t%d\n" % res["reads"], "sampled\t%d\n" % res["sampled"], "adapter\t%s\n" % res["adapter"], "status\t%s\n" % res["status"],
               "seed\t%s\n" % res["seed"], "seed_count\t%d\n" % res["seed_count"], "left_steps\t%d\n" % res["left_steps"],
               "left_stop\t%s\n" % res["left_stop"], "with_adapter\t%d\n" % res["with_adapter"], "dimers\t%d\n" % res["dimers"],
               "insert_mode\t%d\n" % insert_mode(res["insert"])]
    raw, ins, cyc = res["raw_len"].tolist(), res["insert"].tolist(), res["cycles"].tolist()
    last = 0
    for length in range(len(raw)):
        if raw[length] or ins[length][5]:
            last = length
    lengths = ["length\traw\tinserts\tA\tC\tG\tT\tother\n"]
    for length in range(last + 1):
        a, c, g, t, other, total = ins[length]
        lengths.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (length, raw[length], total, a, c, g, t, other))
    cycles = ["cycle\tA\tC\tG\tT\tother\tmean_quality\n"]
    for i, (a, c, g, t, other, qsum) in enumerate(cyc):
        n = a + c + g + t + other
        if n == 0:
            break                          # the reads at cycle i + 1 are among those at cycle i
        milli = (2000 * qsum + n) // (2 * n)       # qsum / n to three decimals, half up, from the integer sums
        cycles.append("%d\t%d\t%d\t%d\t%d\t%d\t%d.%03d\n" % (i + 1, a, c, g, t, other, milli // 1000, milli % 1000))
    return "".join(summary).encode(), "".join(lengths).encode(), "".join(cycles).encode()


def advice(name, res):
    """The line on stdout: the adapter and the trim command that uses it."""
    if res["status"] == "ok":
        return "File %s: adapter %s (ok): python -m mir_prefer_amd.trim -a %s %s\n" % (name, res["adapter"], res["adapter"], name)
    if res["status"] == "unsure":
        return ("File %s: adapter %s (unsure: the walk to its start ended on %s, so it may be an abundant insert, as in a file that is already "
                "trimmed); if it is the adapter: python -m mir_prefer_amd.trim -a %s %s\n" % (name, res["adapter"], res["left_stop"], res["adapter"], name))
    return "File %s: no adapter found (none: no eligible 12-mer occurs 16 times); python -m mir_prefer_amd.trim needs -a from the library's protocol\n" % name


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, files, pm = parse_args(argv)
    for name in files:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the library profile runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        for name in files:
            sys.stdout.write("Start processing file " + name + "\n")
            sys.stdout.flush()
            outs = output_names(name)
            try:
                for path in outs:
                    if os.path.lexists(path):
                        os.remove(path)        # tables of an earlier run: a file that is refused must be left without any
                data = read_input(name)
                res = ctx.libqc_reads(data, name, adapter=options.adapter or "", error_permille=pm, overlap=options.overlap, sample=options.sample)
                del data
                for path, text in zip(outs, render(res)):
                    with open(path, "wb") as f:
                        f.write(text)
            except (ValueError, OSError, capi.MirpError) as e:
                return _fail(str(e))
            sys.stdout.write("Finish file " + name + "\n")
            sys.stdout.write(advice(name, res))
            sys.stdout.flush()
    finally:
        ctx.close()
    sys.stdout.write("DONE\n\n")
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

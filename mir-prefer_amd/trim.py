"""Read trimming before `reads collapse`: the 3' adapter and the low-quality 3' tail are cut from raw reads, FASTQ or FASTA, on the GPU.

    python -m mir_prefer_amd.trim [options] <reads1> ... <readsN>

Every input X gives X.trimmed.fa next to it (a `.gz` suffix is dropped first: lib.fastq.gz gives lib.fastq.trimmed.fa), FASTA that
`python -m mir_prefer_amd.reads collapse` takes as it is.  A `.gz` input is decompressed here, every gzip member in turn.  The files are trimmed in
order, in one device context (mirp_trim_reads, trim_kernels.hip); there is no CPU path.  What is cut and kept is defined in DESIGN.md §13.
With `-a auto` the adapter of every file is found from its reads first, as `python -m mir_prefer_amd.libqc` finds it; a file whose
adapter is not sure (status `unsure` or `none`) is refused like any other refused input.

Option errors exit with status 2 (optparse) before a device is opened; so does -q on a FASTA input.  A missing input, a refused input and "no usable
GPU" print `Error: ...` and exit with status 255; a refused file gets no output, the files before it keep theirs and the files after it are not
processed."""
import gzip
import os
import re
import sys
import zlib
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.trim [options] <reads1> ... <readsN>

    Trim the 3' adapter and low-quality 3' tails from raw small-RNA reads on the GPU.

    The input is FASTQ (Phred+33) or FASTA, plain or gzip-compressed. Every input X gives
    X.trimmed.fa (X without a .gz suffix) next to it, in the format that
    'python -m mir_prefer_amd.reads collapse' reads.

    Example:
    python -m mir_prefer_amd.trim -a TGGAATTCTCGGGTGCCAAGG -q 20 lib1.fastq.gz lib2.fastq.gz
"""
ADAPTER_MAX = 64
AUTO = "auto"          # -a auto: the adapter of every file is found from its reads first (the detection of mir_prefer_amd.libqc)
STATS = ("reads", "quality_trimmed", "adapter", "untrimmed", "too_short", "too_long", "written")


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.trim")
    parser.add_option("-a", "--adapter", help="3' adapter, 1..64 characters of ACGT (either case), or 'auto': found from each file's reads, as "
                      "'python -m mir_prefer_amd.libqc' finds it; a file without a sure adapter is refused. Without -a, no adapter search.")
    parser.add_option("-e", "--error-rate", default="0.1", help="Mismatches allowed per overlap base, 0 <= E < 1, at most three decimals. Default 0.1.")
    parser.add_option("-O", "--overlap", type=int, default=None, help="Minimum overlap with the adapter, 1..len(adapter). Default 3 (at most len(adapter)).")
    parser.add_option("-q", "--quality-cutoff", type=int, default=0, help="3' quality trimming cutoff (Phred+33), 0..93; 0 = off (default). FASTQ only.")
    parser.add_option("-m", "--minimum-length", type=int, default=18, help="Drop reads shorter than this after trimming. Default 18.")
    parser.add_option("-M", "--maximum-length", type=int, default=0, help="Drop reads longer than this after trimming; 0 = off (default).")
    parser.add_option("--discard-untrimmed", action="store_true", help="Drop reads in which no adapter was found (needs -a).")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_permille(text):
    """E as an exact integer in per-mille ("0.1" -> 100), or None when it is not a decimal 0 <= E < 1 with at most three decimals."""
    m = re.fullmatch(r"([0-9]*)(?:\.([0-9]{0,3}))?", text or "")
    if not m or (m.group(1) == "" and not m.group(2)):
        return None
    pm = int(m.group(1) or "0") * 1000 + int((m.group(2) or "").ljust(3, "0"))
    return pm if pm < 1000 else None


def output_name(path):
    return (path[:-3] if path.endswith(".gz") else path) + ".trimmed.fa"


def first_byte(path):
    """The first byte of the (decompressed) file, b"" when empty or unreadable."""
    try:
        if path.endswith(".gz"):
            with gzip.open(path, "rb") as f:
                return f.read(1)
        with open(path, "rb") as f:
            return f.read(1)
    except (OSError, EOFError, zlib.error):
        return b""


def read_input(path):
    """The file's bytes; a `.gz` file decompressed, every member in turn (BGZF too).  Raises ValueError on a corrupt stream."""
    with open(path, "rb") as f:
        data = f.read()
    if not path.endswith(".gz"):
        return data
    try:
        return gzip.decompress(data)
    except (OSError, EOFError, zlib.error) as e:
        raise ValueError("%s: corrupt gzip stream (%s)" % (path, e))


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, files, error_permille, overlap)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 1:
        parser.error("incorrect number of arguments. Run with -h to see the help.")
    adapter = options.adapter
    if adapter is not None and adapter != AUTO and (not 1 <= len(adapter) <= ADAPTER_MAX or re.fullmatch(r"[ACGTacgt]+", adapter) is None):
        parser.error("Option -a must be 1..64 characters of ACGT, or 'auto'.")
    pm = parse_permille(options.error_rate)
    if pm is None:
        parser.error("Option -e must be a decimal 0 <= E < 1 with at most three decimals.")
    m = ADAPTER_MAX if adapter == AUTO else len(adapter) if adapter else 0          # auto: -O is checked against the found adapter per file
    if options.overlap is None:
        overlap = min(3, m) if m else 3
    else:
        overlap = options.overlap
        if not adapter:
            parser.error("Option -O needs -a.")
        if not 1 <= overlap <= m:
            parser.error("Option -O must be between 1 and the adapter length (%d)." % m)
    if not 0 <= options.quality_cutoff <= 93:
        parser.error("Option -q must be between 0 and 93.")
    if options.minimum_length < 0:
        parser.error("Option -m must be at least 0.")
    if options.maximum_length < 0 or (options.maximum_length > 0 and options.maximum_length < options.minimum_length):
        parser.error("Option -M must be 0 or at least -m.")
    if options.discard_untrimmed and not adapter:
        parser.error("Option --discard-untrimmed needs -a.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.quality_cutoff > 0:
        for name in args:
            if os.path.isfile(name) and first_byte(name) == b">":
                parser.error("Option -q needs FASTQ input: %s is FASTA." % name)
    return options, args, pm, overlap


def _fail(msg):
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def found_adapter(ctx, data, name, overlap):
    """-a auto: the adapter of one file's bytes by the detection of `libqc` (capi.Context.libqc_reads, default sample).  Only status `ok` is
    used; anything else, or an -O beyond the found adapter, raises ValueError with the status, the candidate and the advice to run libqc."""
    res = ctx.libqc_reads(data, name)
    if res["status"] != "ok":
        raise ValueError("%s: -a auto found no sure adapter (status %s, candidate %s); run 'python -m mir_prefer_amd.libqc %s' to see the library, "
                         "then give the adapter with -a" % (name, res["status"], res["adapter"] or "-", name))
    if overlap > len(res["adapter"]):
        raise ValueError("%s: Option -O (%d) is larger than the adapter that -a auto found (%s)" % (name, overlap, res["adapter"]))
    sys.stderr.write("File %s: -a auto found the adapter %s\n" % (name, res["adapter"]))
    sys.stderr.flush()
    return res["adapter"]


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, files, pm, overlap = parse_args(argv)
    for name in files:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("trimming runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        for name in files:
            sys.stdout.write("Start processing file " + name + "\n")
            sys.stdout.flush()
            try:
                if os.path.lexists(output_name(name)):
                    os.remove(output_name(name))        # an output of an earlier run: a file that is refused must be left without one
                data = read_input(name)
                adapter = found_adapter(ctx, data, name, overlap) if options.adapter == AUTO else options.adapter or ""
                res = ctx.trim_reads(data, name, output_name(name), adapter=adapter, error_permille=pm, overlap=overlap,
                                     quality=options.quality_cutoff, min_length=options.minimum_length, max_length=options.maximum_length,
                                     discard_untrimmed=bool(options.discard_untrimmed))
            except (ValueError, OSError, capi.MirpError) as e:
                return _fail(str(e))
            del data
            sys.stdout.write("Finish file " + name + "\n")
            sys.stdout.write("File %s: %d reads, %d quality-trimmed, %d with adapter, %d untrimmed discarded, %d too short, %d too long, %d written\n"
                             % ((name,) + tuple(res[k] for k in STATS)))
            sys.stdout.flush()
    finally:
        ctx.close()
    sys.stdout.write("DONE\n\n")
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Read alignment before the pipeline: the reference's scripts/bowtie-align-reads.py, with the alignment on the GPU instead of bowtie.

    python -m mir_prefer_amd.align [options] <read fasta1> ... <read fastaN>

Every read file X (collapsed reads, ids `sample_rA_xN`) gives X.sam next to it.  The options are the script's (-r, -i, -t, -v, -k, -p, -f) plus -m
(the README's direct `bowtie -m`) and --device.  The reference FASTA files (-r) are indexed once per invocation on the device (mirp_align_index) and
every read file is aligned against that index in the same device context (mirp_align_reads); there is no CPU path.  What is reported is defined in
DESIGN.md §12: only the best stratum of hits with at most -v mismatches, the first -k of them in (contig, offset, + before -) order.  With --place u|r (and --window,
--seed) every read is reported once: a multi-mapped read goes to one of its best hits, chosen by the depth of the file's uniquely mapped reads
around each hit or at random (§12 "Placement", ShortStack's --mmap u / r).  With --tail T (and --tail-min, --tail-trim) the reads that find no
such hit are searched for a templated 5' part followed by 1..T non-templated 3' bases (§12 "Tails"): their records carry the clipped tail in
XT:Z:, and X.sam.tails.tsv counts the tails of the file.  -v 0 is the natural partner of --tail: a read that aligns end to end with
substitutions is never reported as tailed.

-i cannot be served (a bowtie index cannot be read): it passes the script's checks and is then refused.  -p is accepted and ignored.  -t is
accepted and the folder created, as the script does; no index files are written there.  Argument errors exit before a device is opened: option
errors with status 2 (optparse), read ids that fail the script's check with status 255."""
import os
import re
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.align [options] <read fasta1> ... <read fastaN>

    Align fasta format reads to genome on the GPU.

    The input fasta format should follow the output of
    'python -m mir_prefer_amd.reads collapse'. That is, the read should be collapsed; the read ID
    must be in format of 'samplename_rA_xN'. Here samplename is the name of the
    sample from with small RNASeq library came from, 'A' is an unique number to
    identify the read, 'N' is the depth of the read.

    The output are SAM format alignment files, which can be then used
    in the pipeline to do miRNA prediction. The output are in the same folder as
    the input files, with suffix ".sam".

    Example:
    python -m mir_prefer_amd.align -k 20 -f -r TAIR10.fa SAMPLE1.fa.processed
"""

READID_ERROR = ("The ID for each read in the output files has the following format: SampleName_rA_xN. Here A is an number uniquely identifies the "
                "read, N is the total count of the read (depth of the read). 'SampleName' is the name of the sample/tissue/library that the input "
                "fasta file represents. For example, if the sample name is 'root', and the read occurred 120 times in the library, then it's "
                "identifier could be root_r23_x120. Here '23' is just a number that donates the order of the reads when processing it, it has no "
                "use otherwise.\n")
PLACE_M = 50            # -m where --place is given without it
PLACE_WINDOW = 50       # --window where --place is given without it
TAIL_MIN = 16           # --tail-min where --tail is given without it
READID_HINT = ("Please use the provided scripts(process-reads-fasta.py, convert-mirdeep2-fasta.py, convert-readcount-file.py) to preprocess the "
               "read fasta files. Refer to the README file for more information.\n\n")


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.align")
    parser.add_option("-r", "--reference", action="append",
                      help="Reference genome in fasta format. If you have multiple reference files, please use multipe -r options.")
    parser.add_option("-i", "--index", help="A bowtie index (checked as the script does, then refused: pass the reference FASTA with -r).")
    parser.add_option("-t", "--temp", help="Temporary folder (created if missing; the index lives on the device, nothing is written there). Only used with -r.")
    parser.add_option("-v", "--allowedmismatch", type=int, default=0, help="Number of mismatches allowed, 0..3. Default is 0.")
    parser.add_option("-k", "--multialignment", type=int, default=20, help="Report up to <int> valid alignments. Default is 20.")
    parser.add_option("-m", "--maxmultialignment", type=int, default=None,
                      help="Report reads with more than <int> alignments in their best stratum as unaligned (XM:i:<int+1>). Default: off.")
    parser.add_option("-p", "--processor", type=int, default=1, help="Accepted for compatibility and ignored.")
    parser.add_option("-f", "--filterunmapped", action="store_true", help="Filter out unmapped alignments in the output.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    parser.add_option("--place", type="choice", choices=["u", "r"], default=None,
                      help="Report every read once. A read with several best alignments goes to one of them: 'u' by the depth of the uniquely "
                           "mapped reads of its file around each alignment (at random where there are none), 'r' always at random. -m then "
                           "defaults to 50 (1..10000) and -k is not consulted. Default: off.")
    parser.add_option("--window", type=int, default=None, help="With --place: bases on each side of an alignment in which uniquely mapped reads count, 0..10000. Default is 50.")
    parser.add_option("--seed", type=int, default=None, help="With --place: seed of the draw, 0..2^64-1. Default is 0.")
    parser.add_option("--tail", type=int, default=None,
                      help="Search the reads without an alignment for a templated 5' part followed by up to <int> (1..8) non-templated 3' bases "
                           "(uridylation, adenylation). Such a read is reported with the tail soft-clipped and named in XT:Z:, and "
                           "<read file>.sam.tails.tsv counts the tails. Best used with -v 0. Not with --place. Default: off.")
    parser.add_option("--tail-min", dest="tail_min", type=int, default=None,
                      help="With --tail: the templated part has at least <int> bases, 12..1024. Default is 16.")
    parser.add_option("--tail-trim", dest="tail_trim", action="store_true",
                      help="With --tail: write the templated part only (SEQ, QUAL and CIGAR without the tail), for stages that take a read's length from SEQ.")
    return parser


def parse_args(argv):
    """The script's parse_option_optparse, plus the range checks of -v, -k, -m and --device; parser.error exits with status 2."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 1:
        parser.error("incorrect number of arguments. Run the script with -h option to see help.")
    if options.reference and options.index:
        parser.error("Options -r and -i are mutually exclusive. Please use only one of them.")
    if not options.reference and not options.index:
        parser.error("Either option -r or -i should be provided.")
    if options.index and options.temp:
        parser.error("Option -t is not needed for option '-r'")
    if not 0 <= options.allowedmismatch <= 3:
        parser.error("Option -v must be between 0 and 3.")
    if options.multialignment < 1:
        parser.error("Option -k must be at least 1.")
    if options.maxmultialignment is not None and options.maxmultialignment < 1:
        parser.error("Option -m must be at least 1.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.place is None:
        if options.window is not None:
            parser.error("Option --window needs --place.")
        if options.seed is not None:
            parser.error("Option --seed needs --place.")
    else:
        if options.maxmultialignment is None:
            options.maxmultialignment = PLACE_M
        if not 1 <= options.maxmultialignment <= 10000:
            parser.error("Option -m must be between 1 and 10000 with --place.")
        if options.window is None:
            options.window = PLACE_WINDOW
        if not 0 <= options.window <= 10000:
            parser.error("Option --window must be between 0 and 10000.")
        if options.seed is None:
            options.seed = 0
        if not 0 <= options.seed < 2 ** 64:
            parser.error("Option --seed must be between 0 and 2^64-1.")
    if options.tail is None:
        if options.tail_min is not None:
            parser.error("Option --tail-min needs --tail.")
        if options.tail_trim:
            parser.error("Option --tail-trim needs --tail.")
    else:
        if options.place is not None:
            parser.error("Options --tail and --place cannot be combined.")
        if not 1 <= options.tail <= 8:
            parser.error("Option --tail must be between 1 and 8.")
        if options.tail_min is None:
            options.tail_min = TAIL_MIN
        if not 12 <= options.tail_min <= 1024:
            parser.error("Option --tail-min must be between 12 and 1024.")
    if options.reference:
        for name in options.reference:
            if not os.path.exists(os.path.abspath(os.path.expanduser(name))):
                parser.error("File " + name + " in option -r does not exist!!")
    if options.index:
        for s in ["1.ebwt", "2.ebwt", "3.ebwt", "4.ebwt", "rev.1.ebwt", "rev.2.ebwt"]:
            name = options.index + "." + s
            if not os.path.exists(os.path.abspath(os.path.expanduser(name))):
                parser.error("Index file " + name + " does not exist!! Please use the -r option instead.")
    for name in args:
        if not os.path.exists(os.path.abspath(os.path.expanduser(name))):
            parser.error("File " + name + " does not exist!!")
    return options, args


def check_readid(readname):
    """The script's check: the headers before the 2,000th must match ^>\\S+_r[0-9]+_x[0-9]+$."""
    count = 0
    pattern = r"^>\S+_r[0-9]+_x[0-9]+$"
    with open(readname, encoding="utf-8", errors="surrogateescape") as f:
        for line in f:
            if line.startswith(">"):
                count += 1
                if count >= 2000:
                    break
                if not re.match(pattern, line.strip()):
                    return False
    return True


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, args = parse_args(argv)
    allgood = True
    for name in args:
        if not check_readid(name):
            sys.stderr.write("ERROR: The format of the read IDs in file " + name + " is not right.\n\n")
            sys.stderr.write(READID_ERROR)
            sys.stderr.write(READID_HINT)
            allgood = False
    if not allgood:
        return 255
    if options.index:
        sys.stderr.write("Error: option -i cannot be used: a bowtie index cannot be read here. Pass the reference FASTA file(s) with -r instead; "
                         "the index is built on the GPU.\n")
        return 255
    if options.temp:
        tempfolder = os.path.expanduser(options.temp)
        if not os.path.exists(tempfolder):
            os.makedirs(tempfolder)
    m = options.maxmultialignment or 0
    cl = " ".join(["python", "-m", "mir_prefer_amd.align"] + argv).replace("\t", " ").replace('"', "'")

    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        sys.stderr.write("Error: alignment runs on the GPU and none is usable (%s); there is no CPU path.\n" % e)
        return 255
    outnames = []
    try:
        sys.stdout.write("\nIndexing reference genomes: " + " ".join(options.reference) + "\n")
        sys.stdout.flush()
        try:
            ctx.align_index(options.reference)
        except capi.MirpError as e:
            sys.stderr.write("Error occurred when indexing reference sequences: %s\n" % e)
            return 255
        for name in args:
            outname = name + ".sam"
            print("SAM file: " + outname)
            sys.stdout.write("\nMapping file " + name + "\n")
            sys.stdout.flush()
            try:
                if options.place:
                    res = ctx.align_reads(name, outname, cl, options.allowedmismatch, options.multialignment, m, bool(options.filterunmapped),
                                          place=options.place, window=options.window, seed=options.seed)
                elif options.tail:
                    res = ctx.align_reads(name, outname, cl, options.allowedmismatch, options.multialignment, m, bool(options.filterunmapped),
                                          tail=options.tail, tail_min=options.tail_min, tail_trim=bool(options.tail_trim))
                else:
                    ctx.align_reads(name, outname, cl, options.allowedmismatch, options.multialignment, m, bool(options.filterunmapped))
            except capi.MirpError as e:
                sys.stderr.write("Error occurred when mapping reads: %s\n" % e)
                return 255
            if options.place:
                sys.stdout.write("Placed: %d unique, %d by density, %d at random, %d suppressed\n"
                                 % (res["unique"], res["by_density"], res["at_random"], res["suppressed"]))
                sys.stdout.flush()
            if options.tail:
                sys.stdout.write("Tailed: %d reads, %d suppressed\n" % (res["tailed"], res["tail_suppressed"]))
                sys.stdout.flush()
            outnames.append(outname)
    finally:
        ctx.close()
    sys.stdout.write("===============================================\nDONE\n")
    sys.stdout.write("Output SAM files can be found at:\n")
    for name in outnames:
        sys.stdout.write(name + "\n")
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

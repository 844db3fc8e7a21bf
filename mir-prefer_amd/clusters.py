"""Small-RNA clusters: where the reads of aligned small-RNA samples lie, with their dominant Dicer size, strand and a count per sample, on the GPU.

    python -m mir_prefer_amd.clusters [options] <sam> [<sam2> ...]

Writes <base>.tsv (one line per cluster), <base>.counts.tsv (a cluster x sample count matrix, the input of differential expression) and
<base>.gff3 (one sRNA_cluster feature per cluster, usable as the pipeline's GFF_FILE_INCLUDE / GFF_FILE_EXCLUDE).  The SAM files are ingested
on the device and stay resident; coverage, islands, clusters, the read assignment and every per-cluster sum run there (mirp_cluster_scan,
clusters_kernels.hip).  This module turns -m into the integer threshold, makes the strand and Dicer calls and writes the files.  DESIGN.md §16
defines it all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused SAM or genome and "no usable GPU" print
`Error: ...` and exit with status 255; a refused run leaves none of the three files, not even ones from an earlier run."""
import os
import re
import sys
from fractions import Fraction
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.clusters [options] <sam> [<sam2> ...]

    Find small-RNA clusters in aligned small-RNA reads on the GPU and count their reads per sample.

    Positions covered by at least -m reads form islands; islands of one contig closer than
    --pad merge into clusters. Every read counts in the first cluster it overlaps. Each SAM
    file is one sample (one column of the count matrix).

    Example:
    python -m mir_prefer_amd.clusters -m 0.5rpm -g genome.fa sample1.sam sample2.sam
"""

TSV_HEADER = (b"name\tcontig\tstart\tend\treads\tplus_reads\tstrand\tdicer_call\tplacements\tmajor_pos\tmajor_strand\tmajor_len\tmajor_reads\t"
              b"major_rna\tshort\tr20\tr21\tr22\tr23\tr24\tlong\n")
GFF_HEADER = b"##gff-version 3\n"
MAX_PAD = 10 ** 6
_DECIMAL = r"([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?"


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.clusters")
    parser.add_option("-m", "--min-coverage", default="0.5rpm",
                      help="Coverage of an island position: a whole number of reads (20) or reads per million of all reads (0.5rpm). Default 0.5rpm.")
    parser.add_option("--pad", type=int, default=75, help="Largest gap in nt between islands of one cluster, 0..1000000. Default 75.")
    parser.add_option("-o", "--output", help="Output base: <base>.tsv, <base>.counts.tsv, <base>.gff3 (a trailing .tsv is removed). "
                                             "Default <first sam>.clusters.")
    parser.add_option("-g", "--genome", help="Genome FASTA: fill major_rna with the major placement's sequence.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def parse_min_coverage(text):
    """-m as ("reads", int >= 1) or ("rpm", Fraction > 0), or None."""
    text = text or ""
    if re.fullmatch(r"[0-9]+", text):
        v = int(text)
        return ("reads", v) if v >= 1 else None
    if text.endswith("rpm") and re.fullmatch(_DECIMAL, text[:-3]):
        v = Fraction(text[:-3])
        return ("rpm", v) if v > 0 else None
    return None


def threshold(spec, total):
    """The integer coverage T: the number of reads, or max(1, ceil(X * total / 10^6)) for X rpm, exactly."""
    kind, x = spec
    if kind == "reads":
        return x
    v = x * total / 10 ** 6
    return max(1, -((-v.numerator) // v.denominator))


def output_base(out, sam_path):
    if out is None:
        return sam_path + ".clusters"
    return out[:-4] if out.endswith(".tsv") else out


def output_paths(base):
    return [base + ".tsv", base + ".counts.tsv", base + ".gff3"]


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, SAM files, -m spec, output base)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if not args:
        parser.error("incorrect number of arguments: at least one SAM file. Run with -h to see the help.")
    spec = parse_min_coverage(options.min_coverage)
    if spec is None:
        parser.error("Option -m must be a whole number of reads of at least 1 or a decimal number greater than 0 followed by rpm (0.5rpm).")
    if not 0 <= options.pad <= MAX_PAD:
        parser.error("Option --pad must be between 0 and %d." % MAX_PAD)
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if options.genome == "":
        parser.error("Option -g needs a file name.")
    return options, args, spec, output_base(options.output, args[0])


# ---------------------------------------------------------------------------------------------------- calls and files
def strand_call(reads, plus):
    if 5 * plus >= 4 * reads:
        return "+"
    if 5 * plus <= reads:
        return "-"
    return "."


def dicer_call(reads, sizes):
    """sizes: depth of len < 20, 20, 21, 22, 23, 24, > 24."""
    dicer = sizes[1:6]
    if 5 * sum(dicer) < 4 * reads:
        return "N"
    top = max(dicer)
    if dicer.count(top) > 1:
        return "N"
    return str(20 + dicer.index(top))


_COMPLEMENT = bytes.maketrans(b"ATGCU", b"UACGA")      # get_complement of the reference


def placement_rna(seq, pos, strand, length):
    """The genome bytes under a placement (within the contig), upper-cased, T -> U; on the minus strand reverse-complemented."""
    s = bytes(seq[max(pos - 1, 0):max(pos - 1 + length, 0)]).upper()
    if strand:
        return s.translate(_COMPLEMENT)[::-1]
    return s.replace(b"T", b"U")


def format_files(contig_names, clusters, counts, sample_names, seqs=None):
    """clusters: CLUSTER_DTYPE array (capi.py) in (tid, start) order; counts: [clusters, samples] depths; seqs[tid]: contig bytes or None.
    -> the bytes of <base>.tsv, <base>.counts.tsv and <base>.gff3."""
    tsv, cnt, gff = [TSV_HEADER], [("name\t" + "\t".join(sample_names) + "\n").encode()], [GFF_HEADER]
    cols = [clusters[f].tolist() for f in ("tid", "start", "end", "reads", "plus_reads", "placements", "major_pos", "major_strand", "major_len",
                                           "major_reads")]
    sizes = clusters["sizes"].tolist()
    rows = counts.tolist()
    for k, (tid, start, end, reads, plus, placements, mpos, mstrand, mlen, mreads) in enumerate(zip(*cols)):
        name = "Cluster_%d" % (k + 1)
        contig = contig_names[tid]
        sc, dc = strand_call(reads, plus), dicer_call(reads, sizes[k])
        rna = placement_rna(seqs[tid], mpos, mstrand, mlen).decode("latin-1") if seqs is not None else "*"
        tsv.append(("%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s\t%s\n"
                    % (name, contig, start, end, reads, plus, sc, dc, placements, mpos, "+-"[mstrand], mlen, mreads, rna,
                       "\t".join(str(x) for x in sizes[k]))).encode("latin-1"))
        cnt.append(("%s\t%s\n" % (name, "\t".join(str(x) for x in rows[k]))).encode())
        gff.append(("%s\tmir_prefer_amd\tsRNA_cluster\t%d\t%d\t.\t%s\t.\tID=%s;DicerCall=%s;Reads=%d\n"
                    % (contig, start, end, sc, name, dc, reads)).encode("latin-1"))
    return b"".join(tsv), b"".join(cnt), b"".join(gff)


# ---------------------------------------------------------------------------------------------------- command line
def _fail(msg, paths=()):
    for p in paths:
        try:
            os.remove(p)
        except OSError:
            pass
    sys.stderr.write("Error: " + msg + "\n")
    sys.stderr.flush()
    return 255


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, sams, spec, base = parse_args(argv)
    outs = output_paths(base)
    for name in sams + ([options.genome] if options.genome else []):
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    from . import early
    early.start_context(options.device)     # the device opens and the SAM files are tokenized while numpy imports (early.py)
    early.start_ingest(sams)
    if options.genome:
        early.start_fasta(options.genome)
    from . import capi
    import numpy as np
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("clusters runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        try:
            if early.has_ingest(sams):
                names, lens, samples, alns, _, _ = ctx.ingest_tokenized(sams)
            else:
                names, lens, samples, alns, _, _ = ctx.ingest_sams(sams)
        except ValueError as e:
            return _fail(str(e))
        total = int(alns["depth"].sum(dtype=np.uint64))
        T = threshold(spec, total)
        try:
            clusters, counts, stats = ctx.cluster_scan(T, options.pad, lens, len(sams))
        except capi.MirpError as e:
            return _fail(str(e))
    finally:
        ctx.close()
    seqs = None
    if options.genome:
        try:
            genome = dict(capi.read_fasta(options.genome))
        except ValueError as e:
            return _fail(str(e))
        seqs = []
        for name, ln in zip(names, lens.tolist()):
            s = genome.get(name)
            if s is None:
                return _fail("contig %s of the SAM header is not in %s" % (name, options.genome))
            if len(s) != ln:
                return _fail("contig %s has %d bases in %s but LN:%d in the SAM header" % (name, len(s), options.genome, ln))
            seqs.append(s)
    files = format_files(names, clusters, counts, list(samples), seqs)
    try:
        for p, body in zip(outs, files):
            with open(p, "wb") as f:
                f.write(body)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("clusters: %d records, total %d reads, T %d, %d islands, %d clusters, %d records assigned, written to %s\n"
                     % (stats["records"], total, T, stats["islands"], stats["clusters"], stats["assigned"], outs[0]))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

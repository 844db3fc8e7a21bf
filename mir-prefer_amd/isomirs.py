"""isomiR counts: the reads of aligned small-RNA samples per annotated miRNA and sample, resolved into 5' / 3' variants and 3' non-templated tails, on the GPU.

    python -m mir_prefer_amd.isomirs [options] <mirnas.gff3> <sam> [<sam2> ...]

Writes <base>.tsv (one line per miRNA: reads, canonical, shifted, trimmed, extended and tailed reads, the major isomiR), <base>.counts.tsv (a miRNA x
sample count matrix, the input of differential expression) and <base>.isomirs.tsv (one line per isomiR with its count per sample).  The SAM files may
come from `align` with or without --tail / --tail-trim: a 3' soft clip or an XT:Z: tag is the tail.  The native tokenizer keeps every record's templated
footprint and tail code (mirp_tokenize_sams_tailed); the assignment to a miRNA, the isomiRs and every sum run on the device (mirp_isomir_scan,
isomir_kernels.hip).  This module reads the annotation and writes the files.  DESIGN.md §28 defines it all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused SAM, GFF or genome and "no usable GPU" print
`Error: ...` and exit with status 255; a refused run leaves none of the three files, not even ones from an earlier run."""
import os
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.isomirs [options] <mirnas.gff3> <sam> [<sam2> ...]

    Count the reads of every annotated miRNA (GFF3 lines of type miRNA) per sample on the GPU and resolve
    them into isomiRs: 5' offset, templated 3' offset and 3' non-templated tail. A read counts in the
    miRNA of its strand whose ends are nearest, within --max5 / --max3. Each SAM file is one sample.

    Example:
    python -m mir_prefer_amd.isomirs -g genome.fa example_miRNA.gff3 sample1.sam sample2.sam
"""

TSV_HEADER = ("name\tlabel\tcontig\tstart\tend\tstrand\treads\tcanonical\tshift5\ttrim3\text3\ttailed\ttail_u\ttail_a\tisomirs\tmajor_d5\tmajor_d3\t"
              "major_tail\tmajor_reads\n")
MAX_OFFSET = 15
MAX_LOCI = 1 << 24
MAX_TAIL = 8


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.isomirs")
    parser.add_option("--max5", type=int, default=2, help="Largest 5' offset between a read and its miRNA, 0..15. Default 2.")
    parser.add_option("--max3", type=int, default=4, help="Largest templated 3' offset between a read and its miRNA, 0..15. Default 4.")
    parser.add_option("-g", "--genome", help="Genome FASTA: fill the seq column of <base>.isomirs.tsv.")
    parser.add_option("-o", "--output", help="Output base: <base>.tsv, <base>.counts.tsv, <base>.isomirs.tsv (a trailing .tsv is removed). "
                                             "Default <first sam>.isomirs.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_base(out, sam_path):
    if out is None:
        return sam_path + ".isomirs"
    return out[:-4] if out.endswith(".tsv") else out


def output_paths(base):
    return [base + ".tsv", base + ".counts.tsv", base + ".isomirs.tsv"]


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, GFF file, SAM files, output base)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a GFF3 file and at least one SAM file. Run with -h to see the help.")
    if not 0 <= options.max5 <= MAX_OFFSET:
        parser.error("Option --max5 must be between 0 and %d." % MAX_OFFSET)
    if not 0 <= options.max3 <= MAX_OFFSET:
        parser.error("Option --max3 must be between 0 and %d." % MAX_OFFSET)
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if options.genome == "":
        parser.error("Option -g needs a file name.")
    return options, args[0], args[1:], output_base(options.output, args[1])


# ---------------------------------------------------------------------------------------------------- annotation
def read_gff(path):
    """The miRNA lines of a GFF3 file in file order -> [(name, label, contig, start, end, strand)]; raises ValueError on a refused file.  Lines are
    taken as gffmask._gff_lines takes them (up to ##FASTA, # lines and blank lines skipped); a line is a locus when its third column is miRNA."""
    loci, ids, places = [], set(), set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            if line.startswith("#"):
                if line.startswith("##FASTA"):
                    break
                continue
            if not line.strip():
                continue
            sp = line.rstrip("\r\n").split("\t")
            if len(sp) < 3 or sp[2] != "miRNA":
                continue
            where = "%s line %d" % (path, no)
            if len(sp) < 9:
                raise ValueError("%s: a miRNA line needs 9 columns" % where)
            try:
                start, end = int(sp[3]), int(sp[4])
            except ValueError:
                raise ValueError("%s: start and end must be whole numbers" % where)
            name, label = None, "."
            for part in sp[8].split(";"):
                key, eq, value = part.strip().partition("=")
                if not eq:
                    continue
                if key == "ID" and name is None:
                    name = value
                elif key.lower() == "name" and label == ".":
                    label = value or "."
            if not name:
                raise ValueError("%s: a miRNA line without an ID attribute" % where)
            if name in ids:
                raise ValueError("%s: the ID %s occurs twice" % (where, name))
            if start < 1:
                raise ValueError("%s: miRNA %s starts before position 1" % (where, name))
            if start > end:
                raise ValueError("%s: miRNA %s has its start behind its end" % (where, name))
            if sp[6] not in ("+", "-"):
                raise ValueError("%s: miRNA %s has strand %s, not + or -" % (where, name, sp[6]))
            place = (sp[0], sp[6], start, end)
            if place in places:
                raise ValueError("%s: miRNA %s repeats the place of another miRNA (%s %s %d..%d)" % ((where, name) + place))
            ids.add(name)
            places.add(place)
            loci.append((name, label, sp[0], start, end, sp[6]))
    return loci


def keep_loci(loci, contig_names, contig_lens):
    """The loci on contigs of the SAM header, in file order -> (kept, dropped count); raises ValueError when none remains, one ends beyond its contig or
    there are more than 2^24."""
    ln = {}
    for n, l in zip(contig_names, contig_lens):
        ln.setdefault(n, int(l))
    kept = [l for l in loci if l[2] in ln]
    for name, _, contig, _, end, _ in kept:
        if end > ln[contig]:
            raise ValueError("miRNA %s ends at %d, beyond the end of sequence %s (LN:%d)" % (name, end, contig, ln[contig]))
    if not kept:
        raise ValueError("no miRNA of the GFF file lies on a sequence of the SAM header")
    if len(kept) > MAX_LOCI:
        raise ValueError("more than %d miRNAs" % MAX_LOCI)
    return kept, len(loci) - len(kept)


# ---------------------------------------------------------------------------------------------------- files
def tail_letters(code):
    """Tail code -> its letters ("" for 0): code = (5^t - 5) / 4 + 1 + the letters A C G T N as a base-5 number."""
    code = int(code)
    if code == 0:
        return ""
    t = 1
    while t < MAX_TAIL and code >= (5 ** (t + 1) - 5) // 4 + 1:
        t += 1
    v = code - ((5 ** t - 5) // 4 + 1)
    out = []
    for _ in range(t):
        out.append("ACGTN"[v % 5])
        v //= 5
    return "".join(reversed(out))


def footprint(locus, d5, d3):
    """(pos, length) of the templated part of an isomiR of the locus (name, label, contig, start, end, strand)."""
    _, _, _, start, end, strand = locus
    if strand == "+":
        r5, r3 = start + d5, end + d3
        return r5, r3 - r5 + 1
    r5, r3 = end - d5, start - d3
    return r3, r5 - r3 + 1


def format_files(loci, isomirs, sums, locus_counts, isomir_counts, sample_names, seqs=None):
    """loci: keep_loci's list; isomirs / sums: ISOMIR_DTYPE / ISO_SUM_DTYPE arrays (capi.py); the two count matrices; seqs[contig name]: contig bytes
    or None.  -> the bytes of <base>.tsv, <base>.counts.tsv and <base>.isomirs.tsv."""
    from .clusters import placement_rna
    samples = "\t".join(sample_names)
    tsv, cnt, iso = [TSV_HEADER], ["name\t" + samples + "\n"], ["name\td5\td3\ttail\treads\tseq\t" + samples + "\n"]
    il, i5, i3, it, ir = (isomirs[f].tolist() for f in ("locus", "d5", "d3", "tail", "reads"))
    srow = [sums[f].tolist() for f in ("reads", "canonical", "shift5", "trim3", "ext3", "tailed", "tail_u", "tail_a", "isomirs", "major_reads", "major")]
    lrows = locus_counts.tolist()
    for k, (name, label, contig, start, end, strand) in enumerate(loci):
        vals = [r[k] for r in srow]
        if vals[8]:
            m = vals[10]
            major = "%d\t%d\t%s\t%d" % (i5[m], i3[m], tail_letters(it[m]) or ".", vals[9])
        else:
            major = ".\t.\t.\t0"
        tsv.append("%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (name, label, contig, start, end, strand, "\t".join(str(v) for v in vals[:9]), major))
        cnt.append("%s\t%s\n" % (name, "\t".join(str(v) for v in lrows[k])))
    for q, row in enumerate(isomir_counts.tolist()):
        locus = loci[il[q]]
        tail = tail_letters(it[q])
        if seqs is None:
            seq = "*"
        else:
            pos, length = footprint(locus, i5[q], i3[q])
            seq = placement_rna(seqs[locus[2]], pos, locus[5] == "-", length).decode("latin-1") + tail.lower().replace("t", "u")
        iso.append("%s\t%d\t%d\t%s\t%d\t%s\t%s\n" % (locus[0], i5[q], i3[q], tail or ".", ir[q], seq, "\t".join(str(v) for v in row)))
    return tuple("".join(x).encode("latin-1") for x in (tsv, cnt, iso))


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
    options, gff, sams, base = parse_args(argv)
    outs = output_paths(base)
    for name in [gff] + sams + ([options.genome] if options.genome else []):
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    try:
        loci = read_gff(gff)
    except (OSError, UnicodeDecodeError, ValueError) as e:
        return _fail(str(e))
    from . import early
    early.start_context(options.device)     # the device opens and the SAM files are tokenized while numpy imports (early.py)
    early.start_tailed(sams)
    if options.genome:
        early.start_fasta(options.genome)
    from . import capi
    import numpy as np
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("isomirs runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        try:
            names, lens, samples, alns, tails, skipped = capi.tokenize_sams_tailed(sams)
            kept, dropped = keep_loci(loci, names, lens.tolist())
        except ValueError as e:
            return _fail(str(e))
        tid_of = {}
        for t, n in enumerate(names):
            tid_of.setdefault(n, t)
        arr = np.zeros(len(kept), dtype=capi.ISO_LOCUS_DTYPE)
        arr["tid"] = [tid_of[l[2]] for l in kept]
        arr["strand"] = [l[5] == "-" for l in kept]
        arr["start"] = [l[3] for l in kept]
        arr["end"] = [l[4] for l in kept]
        try:
            isomirs, sums, locus_counts, isomir_counts, stats = ctx.isomir_scan(alns, tails, arr, options.max5, options.max3, len(sams))
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
        seqs = {}
        for name, ln in zip(names, lens.tolist()):
            s = genome.get(name)
            if s is None:
                return _fail("contig %s of the SAM header is not in %s" % (name, options.genome))
            if len(s) != ln:
                return _fail("contig %s has %d bases in %s but LN:%d in the SAM header" % (name, len(s), options.genome, ln))
            seqs.setdefault(name, s)
    files = format_files(kept, isomirs, sums, locus_counts, isomir_counts, list(samples), seqs)
    try:
        for p, body in zip(outs, files):
            with open(p, "wb") as f:
                f.write(body)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("isomirs: %d records kept, %d skipped (cigar), %d skipped (long_tail), %d miRNAs kept / %d dropped, %d records assigned, "
                     "depth %d assigned, %d isomiRs, written to %s\n"
                     % (stats["records"], skipped["cigar"], skipped["long_tail"], len(kept), dropped, stats["assigned"], stats["depth"],
                        stats["isomirs"], outs[0]))
    sys.stderr.write("isomirs: %d miRNAs of the GFF file lie on sequences that are not in the SAM header\n" % dropped if dropped else "")
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

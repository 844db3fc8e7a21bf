"""siRNA duplexes and the 5' overlap signature on given loci: do the reads of the two strands of a locus pair into duplexes of one length with
3' overhangs, as the products of a Dicer cut through double-stranded RNA do?  On the GPU.

    python -m mir_prefer_amd.signature [options] <loci file> <sam> [<sam2> ...]
    python -m mir_prefer_amd.signature --contigs [options] <sam> [<sam2> ...]

Writes <base>.tsv (one line per locus: reads per strand, the peak of the overlap signature with its z-score, the duplexes and the major one),
<base>.overlaps.tsv (the signature H[1 .. K] per locus) and <base>.duplexes.tsv (every duplex with at least --min-reads paired reads).  The SAM
files are pooled, ingested on the device and stay resident; the join of the two strands and every per-locus sum run there
(mirp_signature_scan, signature_kernels.hip).  This module reads the loci with loci.py's readers, derives the peak, the z-score and the
duplex fraction and writes the files.  DESIGN.md §33 defines it all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused loci file, SAM or genome and "no usable GPU"
print `Error: ...` and exit with status 255; a refused run leaves none of the three files, not even ones from an earlier run."""
import math
import os
import sys
from optparse import OptionParser

from . import loci as _loci

HELP = """python -m mir_prefer_amd.signature [options] <loci file> <sam> [<sam2> ...]
       python -m mir_prefer_amd.signature --contigs [options] <sam> [<sam2> ...]

    Find siRNA duplexes and the 5' overlap signature on given loci on the GPU: the intervals of a
    GFF3 file (clusters, inverted, homologs, the pipeline, annotations), a BED file or a phasing
    output, or every contig as a whole (--contigs). A read belongs to a locus when its 5' end lies
    inside it. Reads on opposite strands whose 5' ends overlap by k bases are counted per k
    (a Dicer product of length L peaks at k = L - 2); a duplex is a plus and a minus placement of
    one length with --overhang bases of 3' overhang on both sides. The SAM files are pooled.

    Example:
    python -m mir_prefer_amd.signature -t sRNA_cluster -g genome.fa run1.clusters.gff3 sample1.sam sample2.sam
"""

TSV_HEADER = (b"name\ttype\tcontig\tstart\tend\treads\tplus_reads\tminus_reads\tpeak_overlap\tpeak_reads\tpeak_z\tduplexes\tduplex_reads\t"
              b"duplex_fraction\tmajor_pos\tmajor_len\tmajor_plus\tmajor_minus\tmajor_rna\n")
DUPLEX_HEADER = b"name\tcontig\tpos\tlen\tplus_reads\tminus_reads\tpaired\tplus_rna\tminus_rna\n"
MAX_OVERLAP = 64
MAX_OVERHANG = 8
LOCI_ENDINGS = (".gff3", ".gff", ".bed", ".phas.tsv")


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.signature")
    parser.add_option("--format", default=None, help="Format of the loci file: auto, gff3, bed or phas. auto (the default) takes a name ending in "
                                                     ".bed as BED, one ending in .phas.tsv as a phasing output and anything else as GFF3.")
    parser.add_option("-t", "--type", action="append", help="GFF3 only: keep the lines whose type (column 3) is one of these; may be repeated or "
                                                            "comma-separated. Default: all types.")
    parser.add_option("--contigs", action="store_true", default=False, help="No loci file: one locus per @SQ contig, spanning the whole contig.")
    parser.add_option("--min-len", type=int, default=20, help="Shortest read that is looked at. Default is 20.")
    parser.add_option("--max-len", type=int, default=25, help="Longest read that is looked at. Default is 25.")
    parser.add_option("--max-overlap", type=int, default=30, help="Largest 5'-to-5' overlap K of the signature, 1..64. Default is 30.")
    parser.add_option("--overhang", type=int, default=2, help="3' overhang of a duplex, 0..8 and below --min-len. Default is 2.")
    parser.add_option("--min-reads", type=int, default=5, help="List the duplexes with at least this many paired reads. Default is 5.")
    parser.add_option("-o", "--output", help="Output base: <base>.tsv, <base>.overlaps.tsv, <base>.duplexes.tsv (a trailing .tsv is removed). Default "
                                             "<first sam>.signature.")
    parser.add_option("-g", "--genome", help="Genome FASTA: fill major_rna, plus_rna and minus_rna with the placements' sequences.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_base(out, sam_path):
    if out is None:
        return sam_path + ".signature"
    return out[:-4] if out.endswith(".tsv") else out


def output_paths(base):
    return [base + ".tsv", base + ".overlaps.tsv", base + ".duplexes.tsv"]


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, loci file or None with --contigs, SAM files, types or
    None, output base)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if options.contigs:
        if len(args) < 1:
            parser.error("incorrect number of arguments: --contigs needs at least one SAM file. Run with -h to see the help.")
        if options.format is not None or options.type is not None:
            parser.error("Options --format and -t describe a loci file; --contigs takes none.")
        for name in args:
            if name.endswith(LOCI_ENDINGS):
                parser.error("Option --contigs takes no loci file (%s); give either --contigs or a loci file." % name)
        loci_path, sams = None, args
    else:
        if len(args) < 2:
            parser.error("incorrect number of arguments: a loci file (or --contigs) and at least one SAM file. Run with -h to see the help.")
        loci_path, sams = args[0], args[1:]
    fmt = "auto" if options.format is None else options.format
    if fmt not in _loci.FORMATS:
        parser.error("Option --format must be one of %s." % ", ".join(_loci.FORMATS))
    options.format = fmt
    types = None
    if options.type is not None:
        types = [t for part in options.type for t in part.split(",")]
        if not all(types):
            parser.error("Option -t needs a feature type.")
        if _loci.file_format(fmt, loci_path) != "gff3":
            parser.error("Option -t selects GFF3 feature types; the loci file is not read as GFF3.")
    if not 1 <= options.min_len <= options.max_len <= 65535:
        parser.error("Options --min-len and --max-len must satisfy 1 <= min <= max <= 65535.")
    if not 1 <= options.max_overlap <= MAX_OVERLAP:
        parser.error("Option --max-overlap must be in 1..%d." % MAX_OVERLAP)
    if not 0 <= options.overhang <= MAX_OVERHANG:
        parser.error("Option --overhang must be in 0..%d." % MAX_OVERHANG)
    if options.overhang >= options.min_len:
        parser.error("Option --overhang must be below --min-len.")
    if options.min_reads < 1:
        parser.error("Option --min-reads must be at least 1.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if options.genome == "":
        parser.error("Option -g needs a file name.")
    return options, loci_path, sams, types, output_base(options.output, sams[0])


def contig_loci(contig_names, contig_lens):
    """--contigs: one locus per contig of the SAM header (the first of a repeated name, as the loci readers resolve names), spanning it whole."""
    out, seen = [], set()
    for name, ln in zip(contig_names, contig_lens):
        if name not in seen and ln >= 1:
            out.append((name, "contig", name, 1, int(ln), "."))
        seen.add(name)
    if not out:
        raise ValueError("no sequence of the SAM header has a base")
    return out


# ---------------------------------------------------------------------------------------------------- files
def host_columns(reads, H, duplex_reads):
    """The host side of §33 for one locus, float64: (peak_overlap, peak_reads, peak_z as printed, duplex_fraction as printed).  The peak is the
    first k of the largest H, 0 when every H is 0; the z-score is over k = 1..K with the population sd, NA when the sd is 0 (all H equal)."""
    top = max(H)
    peak = H.index(top) + 1 if top else 0
    if top == min(H):
        z = "NA"
    else:
        vals = [float(h) for h in H]
        mean = sum(vals) / len(vals)
        z = "%.3f" % ((float(top) - mean) / math.sqrt(sum((v - mean) ** 2 for v in vals) / len(vals)))
    return peak, top, z, "%.4f" % (2.0 * duplex_reads / reads) if reads else "NA"


def format_files(kept, rows, H, sites, overhang, seqs=None):
    """kept: the loci (name, type, contig, start, end, strand); rows: SIGNATURE_ROW_DTYPE, one per locus; H: [loci, K]; sites:
    DUPLEX_SITE_DTYPE in (locus, pos, len) order; seqs[contig name]: contig bytes or None.  -> the bytes of <base>.tsv, <base>.overlaps.tsv
    and <base>.duplexes.tsv."""
    from .clusters import placement_rna
    K = H.shape[1]
    tsv, ovl, dup = [TSV_HEADER], [("name\t" + "\t".join(str(k) for k in range(1, K + 1)) + "\n").encode()], [DUPLEX_HEADER]
    cols = [rows[f].tolist() for f in ("reads", "plus_reads", "duplexes", "duplex_reads", "major_pos", "major_len", "major_plus", "major_minus")]
    for (name, kind, contig, start, end, _), h, reads, plus, nd, dreads, mpos, mlen, mplus, mminus in zip(kept, H.tolist(), *cols):
        peak, top, z, frac = host_columns(reads, h, dreads)
        rna = placement_rna(seqs[contig], mpos, 0, mlen).decode("latin-1") if nd and seqs is not None else "*"
        tsv.append(("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n"
                    % (name, kind, contig, start, end, reads, plus, reads - plus, peak, top, z, nd, dreads, frac, mpos, mlen, mplus, mminus,
                       rna)).encode("latin-1"))
        ovl.append(("%s\t%s\n" % (name, "\t".join(str(x) for x in h))).encode("latin-1"))
    for q, pos, ln, dp, dm in zip(*[sites[f].tolist() for f in ("locus", "pos", "len", "plus_reads", "minus_reads")]):
        name, _, contig = kept[q][:3]
        if seqs is not None:
            a, b = (placement_rna(seqs[contig], pos, 0, ln).decode("latin-1"), placement_rna(seqs[contig], pos - overhang, 1, ln).decode("latin-1"))
        else:
            a = b = "*"
        dup.append(("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (name, contig, pos, ln, dp, dm, min(dp, dm), a, b)).encode("latin-1"))
    return b"".join(tsv), b"".join(ovl), b"".join(dup)


# ---------------------------------------------------------------------------------------------------- command line
def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    options, loci_path, sams, types, base = parse_args(argv)
    outs = output_paths(base)
    _fail = _loci._fail
    for name in ([loci_path] if loci_path is not None else []) + sams + ([options.genome] if options.genome else []):
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    loci = None
    if loci_path is not None:
        try:
            loci = _loci.read_loci(loci_path, options.format, types)
        except (OSError, UnicodeDecodeError, ValueError) as e:
            return _fail(str(e))
    from . import early
    early.start_context(options.device)     # the device opens and the SAM files are tokenized while numpy imports (early.py)
    early.start_ingest(sams)
    if options.genome:
        early.start_fasta(options.genome)
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("signature runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        try:
            if early.has_ingest(sams):
                names, lens, _, _, _, _ = ctx.ingest_tokenized(sams)
            else:
                names, lens, _, _, _, _ = ctx.ingest_sams(sams)
            if loci is None:
                kept, dropped = contig_loci(names, lens.tolist()), 0
            else:
                kept, dropped = _loci.keep_loci(loci, names, lens.tolist())
        except ValueError as e:
            return _fail(str(e))
        try:
            rows, H, sites, stats = ctx.signature_scan(_loci.locus_array(kept, names), lens, options.min_len, options.max_len, options.max_overlap,
                                                       options.overhang, options.min_reads)
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
    files = format_files(kept, rows, H, sites, options.overhang, seqs)
    try:
        for p, body in zip(outs, files):
            with open(p, "wb") as f:
                f.write(body)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("signature: %d records, %d kept (%d..%d nt), %d loci kept / %d dropped (sequence not in the SAM header), %d loci with a duplex, "
                     "%d duplexes listed, written to %s\n"
                     % (stats["records"], stats["kept"], options.min_len, options.max_len, len(kept), dropped, int((rows["duplexes"] > 0).sum()),
                        stats["sites"], outs[0]))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

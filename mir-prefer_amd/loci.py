"""Reads on given loci: the reads of aligned small-RNA samples on every interval of a GFF3, BED or phasing file, per sample, on the GPU.

    python -m mir_prefer_amd.loci [options] <loci file> <sam> [<sam2> ...]

Writes <base>.tsv (one line per locus: reads, strand and Dicer calls, placements, the major placement, size classes) and <base>.counts.tsv (a
locus x sample count matrix on a fixed set of loci, the input of differential expression across runs).  The loci may overlap, nest and repeat:
a read counts in every locus it touches.  The SAM files are ingested on the device and stay resident; the interval join and every per-locus sum
run there (mirp_locus_scan, loci_kernels.hip).  This module reads the loci, makes the strand and Dicer calls and writes the files.  DESIGN.md
§31 defines it all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused loci file, SAM or genome and "no usable GPU"
print `Error: ...` and exit with status 255; a refused run leaves neither file, not even ones from an earlier run."""
import os
import re
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.loci [options] <loci file> <sam> [<sam2> ...]

    Count the reads of aligned small-RNA samples on given loci on the GPU: the intervals of a GFF3
    file (clusters, inverted, homologs, the pipeline, miRBase, gene annotations), a BED file or a
    phasing output. A read counts in every locus that it overlaps by at least one position; loci may
    overlap, nest and repeat. Each SAM file is one sample (one column of the count matrix).

    Example:
    python -m mir_prefer_amd.loci -t sRNA_cluster -g genome.fa run1.clusters.gff3 sample1.sam sample2.sam
"""

TSV_HEADER = (b"name\ttype\tcontig\tstart\tend\tlocus_strand\treads\tplus_reads\tstrand\tdicer_call\tplacements\tmajor_pos\tmajor_strand\tmajor_len\t"
              b"major_reads\tmajor_rna\tshort\tr20\tr21\tr22\tr23\tr24\tlong\n")
FORMATS = ("auto", "gff3", "bed", "phas")
MAX_LOCI = 1 << 24
_WHOLE = re.compile(r"[+-]?[0-9]+")
_STRANDS = {"+": "+", "-": "-", ".": ".", "?": "."}


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.loci")
    parser.add_option("--format", default="auto", help="Format of the loci file: auto, gff3, bed or phas. auto (the default) takes a name ending in "
                                                       ".bed as BED, one ending in .phas.tsv as a phasing output and anything else as GFF3.")
    parser.add_option("-t", "--type", action="append", help="GFF3 only: keep the lines whose type (column 3) is one of these; may be repeated or "
                                                            "comma-separated. Default: all types.")
    parser.add_option("-s", "--stranded", action="store_true", default=False,
                      help="Count a read only in loci of its own strand or without a strand.")
    parser.add_option("-o", "--output", help="Output base: <base>.tsv, <base>.counts.tsv (a trailing .tsv is removed). Default <first sam>.loci.")
    parser.add_option("-g", "--genome", help="Genome FASTA: fill major_rna with the major placement's sequence.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_base(out, sam_path):
    if out is None:
        return sam_path + ".loci"
    return out[:-4] if out.endswith(".tsv") else out


def output_paths(base):
    return [base + ".tsv", base + ".counts.tsv"]


def file_format(fmt, path):
    if fmt != "auto":
        return fmt
    return "bed" if path.endswith(".bed") else "phas" if path.endswith(".phas.tsv") else "gff3"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, loci file, SAM files, types or None, output base)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a loci file and at least one SAM file. Run with -h to see the help.")
    if options.format not in FORMATS:
        parser.error("Option --format must be one of %s." % ", ".join(FORMATS))
    types = None
    if options.type is not None:
        types = [t for part in options.type for t in part.split(",")]
        if not all(types):
            parser.error("Option -t needs a feature type.")
        if file_format(options.format, args[0]) != "gff3":
            parser.error("Option -t selects GFF3 feature types; the loci file is not read as GFF3.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if options.genome == "":
        parser.error("Option -g needs a file name.")
    return options, args[0], args[1:], types, output_base(options.output, args[1])


# ---------------------------------------------------------------------------------------------------- loci files
# A locus is (name, type, contig, start, end, strand): 1-based inclusive, strand "+", "-" or "." (none).
def _interval(where, start, end, strand):
    if not (_WHOLE.fullmatch(start) and _WHOLE.fullmatch(end)):
        raise ValueError("%s: start and end must be whole numbers" % where)
    start, end = int(start), int(end)
    if strand not in _STRANDS:
        raise ValueError("%s: strand %s is not +, -, . or ?" % (where, strand))
    return start, end, _STRANDS[strand]


def _check(where, name, start, end, names):
    if start < 1:
        raise ValueError("%s: locus %s starts before position 1" % (where, name))
    if start > end:
        raise ValueError("%s: locus %s has its start behind its end" % (where, name))
    if name in names:
        raise ValueError("%s: the name %s occurs twice (a GFF3 file with sub-features: select one feature type with -t)" % (where, name))
    names.add(name)


def read_gff(path, types=None):
    """The lines of a GFF3 file in file order, as isomirs.read_gff takes them (up to ##FASTA, # lines and blank lines skipped); with `types` only
    those whose third column is one of them.  Raises ValueError on a refused file."""
    loci, names = [], set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            if line.startswith("#"):
                if line.startswith("##FASTA"):
                    break
                continue
            if not line.strip():
                continue
            sp = line.rstrip("\r\n").split("\t")
            where = "%s line %d" % (path, no)
            if len(sp) >= 3 and types is not None and sp[2] not in types:
                continue
            if len(sp) < 9:
                raise ValueError("%s: a GFF3 line needs 9 columns" % where)
            start, end, strand = _interval(where, sp[3], sp[4], sp[6])
            name = None
            for part in sp[8].split(";"):
                key, eq, value = part.strip().partition("=")
                if eq and key == "ID" and value:
                    name = value
                    break
            if name is None:
                name = "%s:%d-%d:%s" % (sp[0], start, end, strand)
            _check(where, name, start, end, names)
            loci.append((name, sp[2], sp[0], start, end, strand))
    return loci


def read_bed(path):
    """The lines of a BED file in file order (track, browser, # and blank lines skipped): start 0-based, end exclusive."""
    loci, names = [], set()
    with open(path) as f:
        for no, line in enumerate(f, 1):
            if line.startswith("#") or line.startswith("track") or line.startswith("browser") or not line.strip():
                continue
            sp = line.rstrip("\r\n").split("\t")
            where = "%s line %d" % (path, no)
            if len(sp) < 3:
                raise ValueError("%s: a BED line needs 3 columns" % where)
            start, end, strand = _interval(where, sp[1], sp[2], sp[5] if len(sp) > 5 else ".")
            start += 1
            name = sp[3] if len(sp) > 3 and sp[3] != "." and sp[3] != "" else "%s:%d-%d" % (sp[0], start, end)
            _check(where, name, start, end, names)
            loci.append((name, ".", sp[0], start, end, strand))
    return loci


def read_phas(path):
    """The loci of a phasing output (triggers.parse_phas, whose errors pass through), named as triggers names them."""
    from . import triggers
    with open(path, "rb") as f:
        rows = triggers.parse_phas(f.read(), path)
    loci, names = [], set()
    for i, (contig, start, end, _) in enumerate(rows):
        name = "%s:%d-%d" % (contig, start, end)
        _check("%s line %d" % (path, i + 2), name, start, end, names)
        loci.append((name, "PHAS", contig, start, end, "."))
    return loci


def read_loci(path, fmt="auto", types=None):
    fmt = file_format(fmt, path)
    if fmt == "bed":
        return read_bed(path)
    if fmt == "phas":
        return read_phas(path)
    return read_gff(path, types)


def keep_loci(loci, contig_names, contig_lens):
    """The loci on contigs of the SAM header, in file order -> (kept, dropped count); raises ValueError when none remains, one ends beyond its
    contig or there are more than 2^24 (as isomirs.keep_loci)."""
    ln = {}
    for n, l in zip(contig_names, contig_lens):
        ln.setdefault(n, int(l))
    kept = [l for l in loci if l[2] in ln]
    for name, _, contig, _, end, _ in kept:
        if end > ln[contig]:
            raise ValueError("locus %s ends at %d, beyond the end of sequence %s (LN:%d)" % (name, end, contig, ln[contig]))
    if not kept:
        raise ValueError("no locus of the loci file lies on a sequence of the SAM header")
    if len(kept) > MAX_LOCI:
        raise ValueError("more than %d loci" % MAX_LOCI)
    return kept, len(loci) - len(kept)


def locus_array(kept, contig_names):
    """keep_loci's list -> the LOCUS_DTYPE array of capi.Context.locus_scan."""
    from . import capi
    import numpy as np
    tid_of = {}
    for t, n in enumerate(contig_names):
        tid_of.setdefault(n, t)
    arr = np.zeros(len(kept), dtype=capi.LOCUS_DTYPE)
    arr["tid"] = [tid_of[l[2]] for l in kept]
    arr["strand"] = ["+-.".index(l[5]) for l in kept]
    arr["start"] = [l[3] for l in kept]
    arr["end"] = [l[4] for l in kept]
    return arr


# ---------------------------------------------------------------------------------------------------- files
def format_files(kept, rows, counts, sample_names, seqs=None):
    """kept: keep_loci's list; rows: CLUSTER_DTYPE array (capi.py), one row per locus; counts: [loci, samples] depths; seqs[contig name]: contig
    bytes or None.  -> the bytes of <base>.tsv and <base>.counts.tsv.  A locus that counts no record has no calls and no major placement."""
    from .clusters import dicer_call, placement_rna, strand_call
    tsv, cnt = [TSV_HEADER], [("name\t" + "\t".join(sample_names) + "\n").encode()]
    cols = [rows[f].tolist() for f in ("reads", "plus_reads", "placements", "major_pos", "major_strand", "major_len", "major_reads")]
    sizes = rows["sizes"].tolist()
    crow = counts.tolist()
    for k, ((name, kind, contig, start, end, strand), reads, plus, placements, mpos, mstrand, mlen, mreads) in enumerate(zip(kept, *cols)):
        if placements:
            sc, dc, ms = strand_call(reads, plus), dicer_call(reads, sizes[k]), "+-"[mstrand]
            rna = placement_rna(seqs[contig], mpos, mstrand, mlen).decode("latin-1") if seqs is not None else "*"
        else:
            sc, dc, ms, rna = ".", "N", ".", "*"
        tsv.append(("%s\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s\t%s\n"
                    % (name, kind, contig, start, end, strand, reads, plus, sc, dc, placements, mpos, ms, mlen, mreads, rna,
                       "\t".join(str(x) for x in sizes[k]))).encode("latin-1"))
        cnt.append(("%s\t%s\n" % (name, "\t".join(str(x) for x in crow[k]))).encode("latin-1"))
    return b"".join(tsv), b"".join(cnt)


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
    options, loci_path, sams, types, base = parse_args(argv)
    outs = output_paths(base)
    for name in [loci_path] + sams + ([options.genome] if options.genome else []):
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    try:
        loci = read_loci(loci_path, options.format, types)
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
        return _fail("loci runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        try:
            if early.has_ingest(sams):
                names, lens, samples, alns, _, _ = ctx.ingest_tokenized(sams)
            else:
                names, lens, samples, alns, _, _ = ctx.ingest_sams(sams)
            kept, dropped = keep_loci(loci, names, lens.tolist())
        except ValueError as e:
            return _fail(str(e))
        try:
            rows, counts, stats = ctx.locus_scan(locus_array(kept, names), lens, len(sams), options.stranded)
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
    files = format_files(kept, rows, counts, list(samples), seqs)
    try:
        for p, body in zip(outs, files):
            with open(p, "wb") as f:
                f.write(body)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("loci: %d records, %d loci kept / %d dropped (sequence not in the SAM header), %d (record, locus) pairs counted, "
                     "%d loci with reads, written to %s\n"
                     % (stats["records"], len(kept), dropped, stats["pairs"], int((rows["placements"] > 0).sum()), outs[0]))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

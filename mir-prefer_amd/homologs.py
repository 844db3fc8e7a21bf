"""Homologs of known miRNAs in a genome: where do known mature miRNAs (a miRBase mature.fa, say) lie in a genome, with a few mismatches, inside a
hairpin that carries them in one arm with a proper miRNA/miRNA* duplex -- the first pass over a newly assembled species without a small-RNA
library, on the GPU.

    python -m mir_prefer_amd.homologs [options] <known_mature.fa> <genome.fa> [<genome2.fa> ...]

Every known sequence is placed in the genome within -v substitutions on both strands (all strata; mirp_homolog_scan, homolog_kernels.hip), the
window of -P nucleotides around each placement is folded, and the structure and duplex rules of the prediction pipeline are applied to the
placement's interval, without reads and without the expression rules.  Writes <known_mature.fa>.homologs.tsv (one line per locus),
<...>.homologs.precursor.fa and <...>.homologs.mature.fa, and a summary to stdout.  DESIGN.md §26 defines the search and every byte of the files.
The host only formats what the device returns; there is no CPU path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves none of the output files, not even one from an earlier run."""
import os
import sys
from optparse import OptionParser

from .annotate import parse_species
from .randfold import parse_fasta

HELP = """python -m mir_prefer_amd.homologs [options] <known_mature.fa> <genome.fa> [<genome2.fa> ...]

    Find homologs of known mature miRNAs (18..26 nt, A C G U/T; e.g. miRBase mature.fa) in a
    genome on the GPU: every placement within -v mismatches on either strand whose flanking
    sequence folds into a hairpin with the placement in one arm and a proper miRNA/miRNA*
    duplex becomes a locus.

    Example:
    python -m mir_prefer_amd.homologs --species ath,osa -v 2 mature.fa genome.fa
"""
HEADER = ("known\tcontig\tstrand\tmature_start\tmature_end\tmature_seq\tmismatches\tarm\tstar_start\tstar_end\tstar_seq\tfold_s\tfold_e\tenergy\t"
          "norm_energy\ttotal_bps\ttotal_dots\tstructure\talso\n")
MIN_LEN, MAX_LEN = 18, 26
FOLD_MODELS = ("vienna-2.1.2", "vienna-1.8.5")
# the codes of get_maturestar_info (a9) as the pipeline's -d files name them; index 0 = the structure passes
MS_CODES = [None, "FAIL_STRUCTURE_MATCHED_BASES", "FAIL_STRUCTURE_MATURE_NOT_IN_FOLD_REGION", "FAIL_STRUCTURE_MATURE_NOT_IN_ONE_ARM",
            "FAIL_STRUCTURE_MATURE_MATCH_SMALL_THAN_14", "FAIL_STRUCTURE_MATURE_STAR_OVERLAP", "FAIL_STRUCTURE_STAR_OUT_OF_FOLD_REGION",
            "FAIL_STRUCTURE_STAR_NOT_IN_ONE_ARM", "FAIL_STRUCTURE_TOO_MANY_BULGE_OR_LOOP", "FAIL_STRUCTURE_MAX_BULGE_LARGE_THAN_2",
            "FAIL_STRUCTURE_TOTAL_LOOP_SIZE_LARGER_THAN_5", "FAIL_STRUCTURE_NUM_BULGE_MORE_THAN_2", "REFERENCE_EXCEPTION"]


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.homologs")
    parser.add_option("-v", "--max-mismatches", type=int, default=1, help="Most mismatches of a placement, 0..3. Default 1.")
    parser.add_option("-P", "--precursor-len", type=int, default=300, help="Length of the window folded around a placement, 60..3000. Default 300.")
    parser.add_option("-m", "--max-placements", type=int, default=100,
                      help="A known sequence with more placements than this is dropped as repeat-like and counted, at least 1. Default 100.")
    parser.add_option("--fold-model", dest="fold_model", default="vienna-2.1.2", choices=list(FOLD_MODELS),
                      help="Which RNALfold the fold reproduces: vienna-2.1.2 (default) or vienna-1.8.5.")
    parser.add_option("--species", help="Comma-separated id prefixes (ath,osa,...): keep only the known sequences whose id starts with one of them and '-'.")
    parser.add_option("-o", "--output", help="Loci file. Default <known_mature.fa>.homologs.tsv. The FASTA files go to the same name with .precursor.fa "
                      "and .mature.fa for .tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_name(known_path):
    return known_path + ".homologs.tsv"


def fasta_names(tsv_path):
    """(<loci file minus a final .tsv>.precursor.fa, <...>.mature.fa)"""
    stem = tsv_path[:-4] if tsv_path.endswith(".tsv") else tsv_path
    return stem + ".precursor.fa", stem + ".mature.fa"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, known file, genome files, species list, (tsv, precursor.fa,
    mature.fa) paths)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a FASTA of known mature miRNAs and at least one genome FASTA. Run with -h to see the help.")
    if not 0 <= options.max_mismatches <= 3:
        parser.error("Option -v must be between 0 and 3.")
    if not 60 <= options.precursor_len <= 3000:
        parser.error("Option -P must be between 60 and 3000.")
    if options.max_placements < 1:
        parser.error("Option -m must be at least 1.")
    species = []
    if options.species is not None:
        species = parse_species(options.species)
        if species is None:
            parser.error("Option --species needs a non-empty, comma-separated list of non-empty prefixes.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    out = options.output or output_name(args[0])
    return options, args[0], args[1:], species, (out,) + fasta_names(out)


def read_known(data, species=()):
    """FASTA bytes of known mature miRNAs -> ([(sequence, [names])], records read, records skipped).  --species comes first (ids that start with a
    listed prefix and '-'); the records it keeps are `read`.  A sequence is upper-cased with U -> T; a length outside 18..26 or a letter other than
    A C G T is skipped and counted.  Equal sequences are one query that carries all their names in file order; the queries stand in the order of
    their first record."""
    queries, index, n_read, skipped = [], {}, 0, 0
    for name, seq in parse_fasta(data):
        if species and not any(name.startswith(p.encode("latin-1") + b"-") for p in species):
            continue
        n_read += 1
        seq = seq.decode("latin-1").upper().replace("U", "T")
        if not MIN_LEN <= len(seq) <= MAX_LEN or seq.strip("ACGT"):
            skipped += 1
            continue
        if seq not in index:
            index[seq] = len(queries)
            queries.append((seq, []))
        queries[index[seq]][1].append(name.decode("latin-1"))
    return queries, n_read, skipped


def interval(window, win_s, win_e, strand, a, b):
    """The letters of the contig interval [a, b) (1-based, exclusive end) on `strand`, cut from the window [win_s, win_e) as it stands on that strand."""
    return window[a - win_s:b - win_s] if strand == 0 else window[win_e - b:win_e - a]


def loci_of(recs, text, also, queries, contig_names):
    """The device's records as the dictionaries the three files are written from."""
    loci = []
    for r in recs:
        ws, we, strand = int(r["win_s"]), int(r["win_e"]), int(r["strand"])
        at = int(r["text_off"])
        window = text[at:at + we - ws].decode("latin-1")
        cut = lambda a, b: interval(window, ws, we, strand, int(a), int(b))
        others = also[int(r["also_off"]):int(r["also_off"]) + int(r["n_also"])]
        loci.append({"names": list(queries[int(r["query"])][1]), "contig": contig_names[int(r["contig"])], "strand": "+-"[strand],
                     "mat_s": int(r["mat_s"]), "mat_e": int(r["mat_e"]), "mature": cut(r["mat_s"], r["mat_e"]), "mismatches": int(r["mismatches"]),
                     "arm": "5p" if int(r["prime5"]) else "3p", "star_s": int(r["star_s"]), "star_e": int(r["star_e"]),
                     "star": cut(r["star_s"], r["star_e"]), "fold_s": int(r["fold_s"]), "fold_e": int(r["fold_e"]),
                     "precursor": cut(r["fold_s"], r["fold_e"]), "energy": int(r["energy"]), "line_len": int(r["line_len"]),
                     "total_bps": int(r["total_bps"]), "total_dots": int(r["total_dots"]),
                     "ss": text[at + we - ws:at + we - ws + int(r["ss_len"])].decode("latin-1"),
                     "also": [(list(queries[int(q)][1]), int(mm)) for q, mm in others]})
    return loci


def locus_id(locus):
    return "%s_%d_%d_%s" % (locus["contig"], locus["fold_s"], locus["fold_e"], locus["strand"])


def table(loci):
    """The loci file: the header and one line per locus, in the loci's order."""
    lines = [HEADER]
    for x in loci:
        also = ";".join("%s:%d" % (",".join(names), mm) for names, mm in x["also"]) or "."
        lines.append("%s\t%s\t%s\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%.2f\t%.6f\t%d\t%d\t%s\t%s\n" % (
            ",".join(x["names"]), x["contig"], x["strand"], x["mat_s"], x["mat_e"], x["mature"], x["mismatches"], x["arm"], x["star_s"], x["star_e"],
            x["star"], x["fold_s"], x["fold_e"], x["energy"] / 100.0, (x["energy"] / 100.0) / x["line_len"], x["total_bps"], x["total_dots"], x["ss"], also))
    return "".join(lines)


def precursor_fasta(loci):
    """One record per distinct precursor id, in the loci's order: two known miRNAs in the arms of one hairpin share their precursor."""
    seen, lines = set(), []
    for x in loci:
        if locus_id(x) not in seen:
            seen.add(locus_id(x))
            lines.append(">%s\n%s\n" % (locus_id(x), x["precursor"]))
    return "".join(lines)


def mature_fasta(loci):
    """One record per locus: the precursor's id, then the known names and the mature's interval as the description; the genomic mature."""
    return "".join(">%s %s %d_%d\n%s\n" % (locus_id(x), ",".join(x["names"]), x["mat_s"], x["mat_e"], x["mature"]) for x in loci)


def summary_text(n_read, n_skipped, stats):
    """The summary on stdout from the parse counts and homolog_last_stats()."""
    lines = ["known sequences read\t%d\n" % n_read, "known sequences skipped\t%d\n" % n_skipped, "queries\t%d\n" % stats["queries"],
             "queries repeat-like\t%d\n" % stats["repeat_like"], "placements\t%d\n" % stats["placements"], "windows folded\t%d\n" % stats["placements"],
             "loci\t%d\n" % stats["loci"], "placements without a passing structure\t%d\n" % (stats["placements"] - stats["passing"])]
    for k in range(1, len(MS_CODES)):
        if stats["fail_codes"][k]:
            lines.append("  %s\t%d\n" % (MS_CODES[k], stats["fail_codes"][k]))
    if stats["no_structure"]:
        lines.append("  no structure\t%d\n" % stats["no_structure"])
    return "".join(lines)


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
    options, known, genomes, species, outs = parse_args(argv)
    for name in [known] + genomes:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for path in outs:
            if os.path.lexists(path):
                os.remove(path)             # outputs of an earlier run: a refused run must be left without them
        with open(known, "rb") as f:
            data = f.read()
    except OSError as e:
        return _fail(str(e))
    try:
        queries, n_read, n_skipped = read_known(data, species)
    except ValueError as e:
        return _fail("%s: %s" % (known, e))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the homolog search runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        ctx.set_fold_model(options.fold_model)
        ctx.align_index(genomes)
        recs, text, also = ctx.homolog_scan([q for q, _ in queries], max_mismatches=options.max_mismatches, precursor_len=options.precursor_len,
                                            max_placements=options.max_placements)
        stats = ctx.homolog_last_stats()
        loci = loci_of(recs, text, also, queries, ctx.align_contigs()[0])
        for path, body in zip(outs, (table(loci), precursor_fasta(loci), mature_fasta(loci))):
            with open(path, "w", encoding="latin-1", newline="") as f:
                f.write(body)
    except (OSError, capi.MirpError) as e:
        _remove(outs)
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stdout.write(summary_text(n_read, n_skipped, stats))
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Known-hairpin comparison: which predicted precursors are members of known MIR families, by gapped local alignment against known hairpins (a
miRBase hairpin.fa, say), on the GPU.

    python -m mir_prefer_amd.hairpins [options] <precursors.fa> <known_hairpins.fa> [<known2.fa> ...]

Every precursor is aligned with every known sequence in the same sense (Gotoh's local alignment with affine gaps; mirp_hairpin_align,
hairpin_kernels.hip).  Writes one tab-separated file of hits (default <precursors.fa>.hairpins.tsv) and one line per precursor to a summary file
beside it.  DESIGN.md §25 defines the alignment, its ties, the order and both files.  The host only formats what the device returns; there is no
CPU path.

Option errors exit with status 2 (optparse) before a device is opened.  A missing input, a refused input and "no usable GPU" print `Error: ...`
and exit with status 255; a refused or failed run leaves neither output file, not even one from an earlier run."""
import os
import re
import sys
from optparse import OptionParser

from .annotate import parse_species, summary_name
from .randfold import parse_fasta

HELP = """python -m mir_prefer_amd.hairpins [options] <precursors.fa> <known_hairpins.fa> [<known2.fa> ...]

    Align precursors (1..3000 nt) with known hairpins (e.g. miRBase hairpin.fa) on the GPU:
    gapped local alignment in the same sense, A C G U/T in either case, any other letter
    mismatches everything. A pair is a hit when its score reaches -s. Each precursor is classed
    identical (the whole of both sequences, no mismatch), homolog (any other hit) or novel.

    Example:
    python -m mir_prefer_amd.hairpins --species ath,osa out/prefix_miRNA.precursor.fa hairpin.fa
"""
HEADER = "query\tknown\tfamily\tscore\tidentity\tq_start\tq_end\tq_len\tk_start\tk_end\tk_len\tmatches\tmismatches\tgap_opens\tgap_bases\tcigar\n"
MAX_LEN = 3000
FAMILY = re.compile(r"^(?:[A-Za-z0-9]+-)?(mir|let|lin)-?([0-9]+)", re.I)


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.hairpins")
    parser.add_option("--match", type=int, default=2, help="Score of a column of two equal letters, 1..10. Default 2.")
    parser.add_option("--mismatch", type=int, default=3, help="Penalty of a column of two different letters, 1..10. Default 3.")
    parser.add_option("--gap-open", type=int, default=5, help="Penalty of opening a gap, 0..20; a gap of g bases costs gap-open + g x gap-extend. Default 5.")
    parser.add_option("--gap-extend", type=int, default=2, help="Penalty of every base of a gap, 1..10. Default 2.")
    parser.add_option("-s", "--min-score", type=int, default=60, help="Smallest score of a hit, at least 1. Default 60.")
    parser.add_option("-k", "--max-hits", type=int, default=0, help="Write the first N hits per query, in output order; 0 = all (default).")
    parser.add_option("--species", help="Comma-separated id prefixes (ath,osa,...): keep only the known sequences whose id starts with one of them and '-'.")
    parser.add_option("-o", "--output", help="Hits file. Default <precursors.fa>.hairpins.tsv. The summary goes to the same name with .summary.tsv for .tsv.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_name(query_path):
    return query_path + ".hairpins.tsv"


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, query file, known files, species list, hits path, summary path)."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) < 2:
        parser.error("incorrect number of arguments: a FASTA of precursors and at least one FASTA of known hairpins. Run with -h to see the help.")
    for name, value, lo, hi in (("--match", options.match, 1, 10), ("--mismatch", options.mismatch, 1, 10), ("--gap-open", options.gap_open, 0, 20),
                                ("--gap-extend", options.gap_extend, 1, 10)):
        if not lo <= value <= hi:
            parser.error("Option %s must be between %d and %d." % (name, lo, hi))
    if options.min_score < 1:
        parser.error("Option -s must be at least 1.")
    if options.max_hits < 0:
        parser.error("Option -k must be at least 0.")
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
    return options, args[0], args[1:], species, out, summary_name(out)


def family(name):
    """The family of a known id by §19's rule: ath-MIR166a -> miR166, cel-let-7 -> let-7, cel-lin-4 -> lin-4; without a match the id itself."""
    m = FAMILY.match(name)
    if not m:
        return name
    kind = m.group(1).lower()
    return ("miR" if kind == "mir" else kind + "-") + m.group(2)


def high_byte_record(data):
    """The 1-based record of the first header or sequence line that holds a byte >= 0x80, or 0; text before the first header is ignored, as
    parse_fasta ignores it."""
    rec = 0
    for line in re.split(rb"\r\n|\r|\n", data):
        if line.startswith(b">"):
            rec += 1
        if rec and any(b >= 0x80 for b in line):
            return rec
    return 0


def read_queries(data):
    """[(name, sequence)] of the query file; ValueError names the 1-based record of a byte >= 0x80 anywhere in a record (the rest of the header
    line included) or of an empty or too long sequence."""
    rec = high_byte_record(data)
    if rec:
        raise ValueError("record %d: a byte >= 0x80" % rec)
    records = parse_fasta(data)
    for r, (name, seq) in enumerate(records):
        why = "an empty sequence" if not seq else "a sequence longer than 3,000 nt" if len(seq) > MAX_LEN else None
        if why:
            raise ValueError("record %d: %s" % (r + 1, why))
    return records


def read_known(datas, species):
    """([(name, sequence)], skipped) of the known files in order: a length outside 1..3000 is skipped and counted, then --species keeps the ids that
    start with a listed prefix and '-'.  ValueError carries (file index, message) for a byte >= 0x80 anywhere in a record, also in one that would
    be skipped or filtered out."""
    kept, skipped = [], 0
    for fi, data in enumerate(datas):
        rec = high_byte_record(data)
        if rec:
            raise ValueError(fi, "record %d: a byte >= 0x80" % rec)
        try:
            records = parse_fasta(data)
        except ValueError as e:
            raise ValueError(fi, str(e))
        for name, seq in records:
            if not 1 <= len(seq) <= MAX_LEN:
                skipped += 1
            elif not species or any(name.startswith(p.encode("latin-1") + b"-") for p in species):
                kept.append((name, seq))
    return kept, skipped


def is_identical(rec, q_len, k_len):
    return int(rec["matches"]) == q_len == k_len and int(rec["mismatches"]) == 0 and int(rec["gap_bases"]) == 0


def hits_table(q_names, q_lens, k_names, k_lens, recs, cigars):
    """The hits file: the header and one line per hit record, in the records' order."""
    lines = [HEADER]
    for rec, cigar in zip(recs, cigars):
        q, k = int(rec["query"]), int(rec["known"])
        m, x, g = int(rec["matches"]), int(rec["mismatches"]), int(rec["gap_bases"])
        lines.append("%s\t%s\t%s\t%d\t%.2f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (
            q_names[q], k_names[k], family(k_names[k]), int(rec["score"]), 100 * m / (m + x + g), int(rec["q_start"]), int(rec["q_end"]), q_lens[q],
            int(rec["k_start"]), int(rec["k_end"]), k_lens[k], m, x, int(rec["gap_opens"]), g, cigar))
    return "".join(lines)


def summary_table(q_names, q_lens, k_names, k_lens, recs, per_query):
    """(the summary file: one line per query in file order from its first record, its hit count before -k and the families of its records,
    {class: queries})."""
    first, fams = {}, {}
    for rec in recs:
        q = int(rec["query"])
        first.setdefault(q, rec)
        f = family(k_names[int(rec["known"])])
        if f not in fams.setdefault(q, []):
            fams[q].append(f)
    lines, classes = [], {"identical": 0, "homolog": 0, "novel": 0}
    for q, name in enumerate(q_names):
        rec = first.get(q)
        if rec is None:
            classes["novel"] += 1
            lines.append("%s\t%d\tnovel\t.\t.\t.\t.\t.\t.\t0\t.\n" % (name, q_lens[q]))
            continue
        k = int(rec["known"])
        m, x, g = int(rec["matches"]), int(rec["mismatches"]), int(rec["gap_bases"])
        cls = "identical" if is_identical(rec, q_lens[q], k_lens[k]) else "homolog"
        classes[cls] += 1
        lines.append("%s\t%d\t%s\t%s\t%s\t%d\t%.2f\t%.2f\t%.2f\t%d\t%s\n" % (
            name, q_lens[q], cls, k_names[k], family(k_names[k]), int(rec["score"]), 100 * m / (m + x + g),
            100 * (int(rec["q_end"]) - int(rec["q_start"]) + 1) / q_lens[q], 100 * (int(rec["k_end"]) - int(rec["k_start"]) + 1) / k_lens[k],
            int(per_query[q]), ",".join(fams[q])))
    return "".join(lines), classes


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
    options, query, known_paths, species, out, summary = parse_args(argv)
    for name in [query] + known_paths:
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for path in (out, summary):
            if os.path.lexists(path):
                os.remove(path)             # outputs of an earlier run: a refused run must be left without them
        with open(query, "rb") as f:
            data = f.read()
        datas = []
        for name in known_paths:
            with open(name, "rb") as f:
                datas.append(f.read())
    except OSError as e:
        return _fail(str(e))
    try:
        queries = read_queries(data)
    except ValueError as e:
        return _fail("%s: %s" % (query, e))
    try:
        known, skipped = read_known(datas, species)
    except ValueError as e:
        return _fail("%s: %s" % (known_paths[e.args[0]], e.args[1]))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("the alignment runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        recs, cigars = ctx.hairpin_align([s for _, s in queries], [s for _, s in known], match=options.match, mismatch=options.mismatch,
                                         gap_open=options.gap_open, gap_extend=options.gap_extend, min_score=options.min_score, max_lines=options.max_hits)
        stats = ctx.hairpin_last_stats()
        q_names, q_lens = [n.decode("latin-1") for n, _ in queries], [len(s) for _, s in queries]
        k_names, k_lens = [n.decode("latin-1") for n, _ in known], [len(s) for _, s in known]
        text, classes = summary_table(q_names, q_lens, k_names, k_lens, recs, stats["per_query"])
        with open(out, "w", encoding="latin-1", newline="") as f:
            f.write(hits_table(q_names, q_lens, k_names, k_lens, recs, cigars))
        with open(summary, "w", encoding="latin-1", newline="") as f:
            f.write(text)
    except (OSError, capi.MirpError) as e:
        _remove((out, summary))
        return _fail(str(e))
    finally:
        ctx.close()
    sys.stderr.write("hairpins: %d queries, %d known sequences kept (%d skipped), %d pairs, %d cells, %d hits; %d identical, %d homolog, %d novel; "
                     "written to %s and %s\n" % (stats["queries"], stats["known"], skipped, stats["pairs"], stats["cells"], stats["hits"],
                                                 classes["identical"], classes["homolog"], classes["novel"], out, summary))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

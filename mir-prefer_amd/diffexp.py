"""Differential expression between two groups of samples: the exact negative-binomial test on a feature x sample count matrix, on the GPU.

    python -m mir_prefer_amd.diffexp -a root1,root2,root3 -b leaf1,leaf2 [options] study.counts.tsv

Reads a <base>.counts.tsv as clusters, isomirs and loci write it and writes <out>.tsv (one line per feature: means, log2 fold change, dispersion,
p and the Benjamini-Hochberg adjusted p), <out>.norm.tsv (the counts divided by the size factors) and <out>.factors.tsv (sample, group, column
sum, size factor).  The moments of every feature and the test -- one term per read of a feature -- run on the device (mirp_diffexp,
diffexp_kernels.hip); this module reads the matrix, makes the size factors, adjusts the p-values and writes the files.  DESIGN.md §32 defines it
all.

Option errors exit with status 2 (optparse) before a device is opened.  A missing or refused matrix or size-factor file, a matrix without a
usable feature and "no usable GPU" print `Error: ...` and exit with status 255; a refused run leaves none of the three files, not even ones from
an earlier run."""
import math
import os
import re
import sys
from optparse import OptionParser

HELP = """python -m mir_prefer_amd.diffexp -a <samples of group A> -b <samples of group B> [options] <matrix.counts.tsv>

    Test every feature of a count matrix (clusters, isomirs, loci) for a difference between two groups
    of samples on the GPU: size factors, a dispersion per feature and the exact negative-binomial
    test of Anders & Huber 2010 (DESeq's nbinomTest), with every split of a feature's reads summed.
    Columns named in neither -a nor -b are ignored.

    Example:
    python -m mir_prefer_amd.diffexp -a root1,root2,root3 -b leaf1,leaf2 study.counts.tsv
"""

TSV_HEADER = b"name\tbaseMean\tmeanA\tmeanB\tlog2fc\tdispersion\tp\tpadj\n"
FACTORS_HEADER = b"sample\tgroup\tcolumn_sum\tsize_factor\n"
NORMS = ("mor", "total", "none")
MODES = ("max", "common", "feature")
MAX_FEATURES = 1 << 24
MAX_COUNT = 1 << 40
MAX_SAMPLES = 255
_WHOLE = re.compile(r"[0-9]+")


def make_parser():
    parser = OptionParser(HELP, prog="mir_prefer_amd.diffexp")
    parser.add_option("-a", "--group-a", action="append", help="Columns of group A; may be repeated or comma-separated.")
    parser.add_option("-b", "--group-b", action="append", help="Columns of group B; may be repeated or comma-separated.")
    parser.add_option("-o", "--output", help="Output base: <base>.tsv, <base>.norm.tsv, <base>.factors.tsv (a trailing .tsv is removed). "
                                             "Default: the matrix without .counts.tsv, plus .diffexp.")
    parser.add_option("--norm", default="mor", help="Size factors: mor (median of ratios, the default), total (column sums over their geometric "
                                                    "mean) or none (all 1).")
    parser.add_option("--size-factors", help="File of `sample<TAB>value` lines with the size factor of every used sample; overrides --norm.")
    parser.add_option("--dispersion", default="max", help="max (the larger of the feature's own and the common dispersion, the default), common, "
                                                          "feature, or a number >= 0 used for every feature (0: the exact binomial test).")
    parser.add_option("--min-mean", type=float, default=10.0, help="The common dispersion is the median over the features with a mean of at least "
                                                                   "this. Default 10.")
    parser.add_option("--pseudo", type=float, default=0.5, help="Added to both means in log2fc. Default 0.5.")
    parser.add_option("--device", type=int, default=0, help="GPU device index. Default is 0.")
    return parser


def output_base(out, matrix):
    if out is None:
        return (matrix[:-len(".counts.tsv")] if matrix.endswith(".counts.tsv") else matrix) + ".diffexp"
    return out[:-4] if out.endswith(".tsv") else out


def output_paths(base):
    return [base + ".tsv", base + ".norm.tsv", base + ".factors.tsv"]


def _finite_nonneg(x):
    return x == x and 0.0 <= x < float("inf")


def parse_args(argv):
    """Options and their checks; parser.error exits with status 2.  Returns (options, matrix, names of A, names of B, (mode, phi), output base);
    mode is an index of capi.DIFFEXP_MODES."""
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if len(args) != 1:
        parser.error("incorrect number of arguments: one count matrix. Run with -h to see the help.")
    groups = []
    for flag, given in (("-a", options.group_a), ("-b", options.group_b)):
        if given is None:
            parser.error("Option %s is required: the columns of the group." % flag)
        names = [n for part in given for n in part.split(",")]
        if not all(names):
            parser.error("Option %s needs column names." % flag)
        if len(set(names)) != len(names):
            parser.error("Option %s names a column twice." % flag)
        groups.append(names)
    a, b = groups
    if set(a) & set(b):
        parser.error("Options -a and -b share the column %s." % sorted(set(a) & set(b))[0])
    if len(a) + len(b) > MAX_SAMPLES:
        parser.error("Options -a and -b name more than %d columns." % MAX_SAMPLES)
    if options.norm not in NORMS:
        parser.error("Option --norm must be one of %s." % ", ".join(NORMS))
    if options.dispersion in MODES:
        mode, phi = MODES.index(options.dispersion), 0.0
        if len(a) == 1 and len(b) == 1:
            parser.error("One sample per group has no variance to estimate a dispersion from: give --dispersion a number (0 is the exact "
                         "binomial test).")
    else:
        try:
            phi = float(options.dispersion)
        except ValueError:
            phi = -1.0
        if not _finite_nonneg(phi):
            parser.error("Option --dispersion must be max, common, feature or a number >= 0.")
        mode = 3
    if not _finite_nonneg(options.min_mean):
        parser.error("Option --min-mean must be a number >= 0.")
    if not _finite_nonneg(options.pseudo):
        parser.error("Option --pseudo must be a number >= 0.")
    if options.device < 0:
        parser.error("Option --device must be at least 0.")
    if options.output == "":
        parser.error("Option -o needs a file name.")
    if options.size_factors == "":
        parser.error("Option --size-factors needs a file name.")
    return options, args[0], a, b, (mode, phi), output_base(options.output, args[0])


# ---------------------------------------------------------------------------------------------------- the matrix
def read_matrix(path, a, b):
    """The used columns of a count matrix, A before B, each in option order -> (feature names, uint64 array [features, len(a) + len(b)]).  Raises
    ValueError `<file> line <n>: ...` on a refused file."""
    import numpy as np
    used = list(a) + list(b)
    names, seen, flat = [], set(), []
    with open(path, encoding="latin-1", newline="") as f:
        header = f.readline()
        if not header.strip("\r\n"):
            raise ValueError("%s line 1: no header line" % path)
        cols = header.rstrip("\r\n").split("\t")
        if len(cols) < 2:
            raise ValueError("%s line 1: the header needs a name column and at least one sample" % path)
        samples = cols[1:]
        if len(set(samples)) != len(samples):
            dup = sorted(s for s in set(samples) if samples.count(s) > 1)[0]
            raise ValueError("%s line 1: the column name %s occurs twice" % (path, dup))
        for s in used:
            if s not in samples:
                raise ValueError("%s line 1: there is no column %s" % (path, s))
        at = [1 + samples.index(s) for s in used]
        width = len(cols)
        for no, line in enumerate(f, 2):
            sp = line.rstrip("\r\n").split("\t")
            if len(sp) != width:
                raise ValueError("%s line %d: %d columns where the header has %d" % (path, no, len(sp), width))
            if sp[0] in seen:
                raise ValueError("%s line %d: the feature name %s occurs twice" % (path, no, sp[0]))
            seen.add(sp[0])
            names.append(sp[0])
            for k in at:
                if not _WHOLE.fullmatch(sp[k]):
                    raise ValueError("%s line %d: %s is not a non-negative whole number" % (path, no, sp[k] if sp[k] else "an empty field"))
                v = int(sp[k])
                if v >= MAX_COUNT:
                    raise ValueError("%s line %d: the count %s is 2^40 or more" % (path, no, sp[k]))
                flat.append(v)
            if len(names) > MAX_FEATURES:
                raise ValueError("%s line %d: more than %d features" % (path, no, MAX_FEATURES))
    return names, np.array(flat, dtype=np.uint64).reshape(len(names), len(used))


def read_size_factors(path, used):
    """`sample<TAB>value` lines -> the values of the used samples in their order.  Raises ValueError."""
    import numpy as np
    table = {}
    with open(path, encoding="latin-1") as f:
        for no, line in enumerate(f, 1):
            if not line.strip():
                continue
            sp = line.rstrip("\r\n").split("\t")
            try:
                v = float(sp[1]) if len(sp) == 2 else float("nan")
            except ValueError:
                v = float("nan")
            if not (v > 0.0 and v < float("inf")):
                raise ValueError("%s line %d: a line is `sample<TAB>size factor`, the factor a number > 0" % (path, no))
            if sp[0] in table:
                raise ValueError("%s line %d: the sample %s occurs twice" % (path, no, sp[0]))
            table[sp[0]] = v
    for s in used:
        if s not in table:
            raise ValueError("%s: no size factor for the sample %s" % (path, s))
    return np.array([table[s] for s in used], dtype=np.float64)


def size_factors(counts, norm):
    """counts: [features, used samples] -> one size factor per sample.  Raises ValueError where the rule has nothing to work on."""
    import numpy as np
    S = counts.shape[1]
    if norm == "none":
        return np.ones(S, dtype=np.float64)
    if norm == "total":
        tot = counts.sum(axis=0, dtype=np.uint64).astype(np.float64)
        if (tot == 0).any():
            raise ValueError("--norm total: a used sample has no read at all")
        ln = np.log(tot)
        return tot / math.exp(float(ln.sum() / S))
    ok = (counts > 0).all(axis=1)
    if not ok.any():
        raise ValueError("--norm mor: no feature has a read in every used sample; --norm total does not need one")
    ln = np.log(counts[ok].astype(np.float64))
    return np.exp(np.median(ln - ln.mean(axis=1, keepdims=True), axis=0))


def adjust(p):
    """Benjamini-Hochberg over the tested features (p >= 0): padj_(k) = min over k' >= k of p_(k') * m / k', capped at 1; -1 where p is -1."""
    import numpy as np
    p = np.asarray(p, dtype=np.float64)
    out = np.full(len(p), -1.0)
    idx = np.flatnonzero(p >= 0)
    m = len(idx)
    if m:
        order = idx[np.argsort(p[idx], kind="stable")]
        scaled = p[order] * m / np.arange(1, m + 1, dtype=np.float64)
        out[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return out


# ---------------------------------------------------------------------------------------------------- files
def _g(x):
    return "NA" if x != x else "%.6g" % x


def _p(x):
    from fractions import Fraction
    from .phasing import pvalue_text
    return "NA" if x < 0 else pvalue_text(Fraction(x))


def format_files(names, counts, used, n_a, sf, rows, padj):
    """-> the bytes of <base>.tsv, <base>.norm.tsv and <base>.factors.tsv.  rows: capi.DIFFEXP_DTYPE; padj: adjust(rows["p"])."""
    import numpy as np
    cols = [rows[f].tolist() for f in ("base_mean", "mean_a", "mean_b", "log2fc", "dispersion", "p")]
    tsv = [TSV_HEADER]
    for name, bm, ma, mb, fc, d, p, pa in zip(names, *cols, padj.tolist()):
        tsv.append(("%s\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n" % (name, _g(bm), _g(ma), _g(mb), _g(fc), _g(d), _p(p), _p(pa))).encode("latin-1"))
    y = counts.astype(np.float64) / sf
    norm = [("name\t" + "\t".join(used) + "\n").encode("latin-1")]
    for name, row in zip(names, y.tolist()):
        norm.append(("%s\t%s\n" % (name, "\t".join("%.3f" % v for v in row))).encode("latin-1"))
    tot = counts.sum(axis=0, dtype=np.uint64).tolist() if len(names) else [0] * len(used)
    fac = [FACTORS_HEADER]
    for j, s in enumerate(used):
        fac.append(("%s\t%s\t%d\t%.10g\n" % (s, "A" if j < n_a else "B", tot[j], sf[j])).encode("latin-1"))
    return b"".join(tsv), b"".join(norm), b"".join(fac)


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
    options, matrix, a, b, (mode, phi), base = parse_args(argv)
    outs = output_paths(base)
    for name in [matrix] + ([options.size_factors] if options.size_factors else []):
        if not os.path.isfile(name):
            return _fail("file " + name + " does not exist!!!")
    try:
        for p in outs:
            if os.path.lexists(p):
                os.remove(p)                # an output of an earlier run: a refused run must be left without one
    except OSError as e:
        return _fail(str(e))
    used = a + b
    try:
        names, counts = read_matrix(matrix, a, b)
        sf = read_size_factors(options.size_factors, used) if options.size_factors else size_factors(counts, options.norm)
    except (OSError, ValueError) as e:
        return _fail(str(e))
    from . import capi
    try:
        ctx = capi.Context(options.device)
    except capi.MirpError as e:
        return _fail("diffexp runs on the GPU and none is usable (%s); there is no CPU path." % e)
    try:
        rows, stats = ctx.diffexp(counts, sf, [0] * len(a) + [1] * len(b), mode, phi, options.min_mean, options.pseudo)
    except capi.MirpError as e:
        return _fail(str(e))
    finally:
        ctx.close()
    padj = adjust(rows["p"])
    files = format_files(names, counts, used, len(a), sf, rows, padj)
    try:
        for p, body in zip(outs, files):
            with open(p, "wb") as f:
                f.write(body)
    except OSError as e:
        return _fail(str(e), outs)
    sys.stderr.write("diffexp: %d features, %d tested, %d terms, common dispersion %.6g, %d features with padj <= 0.05, written to %s\n"
                     % (stats["features"], stats["tested"], stats["terms"], stats["phi_c"], int(((padj >= 0) & (padj <= 0.05)).sum()), outs[0]))
    sys.stderr.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())

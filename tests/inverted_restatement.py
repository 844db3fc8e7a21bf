"""Restatement of the inverted-repeat search, twice: the recurrence cell by cell in plain Python, and level by level in numpy.
Both share the candidate rule, the traceback, the selection and the three writers, which read H through a function of (i, j).  Positions are
1-based as in the definition.  Nothing here is fast, and nothing here is imported by the package."""
import numpy as np

PAIRS = {("A", "T"), ("T", "A"), ("C", "G"), ("G", "C")}
DEFAULTS = dict(max_span=2000, min_score=50, match=3, mismatch=4, gap=12)
TSV_HEADER = ("name\tcontig\tstart\tend\tscore\tleft_start\tleft_end\tright_start\tright_end\tloop\tmatches\tmismatches\tgaps\tidentity\t"
              "structure\n")


def letters(seq):
    """bytes / str -> a str over ACGTN: either case, U as T, every other byte N; a byte >= 0x80 is refused."""
    data = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    out = []
    for ch in data:
        if ch >= 0x80:
            raise ValueError("a byte >= 0x80")
        c = chr(ch).upper()
        out.append("T" if c == "U" else c if c in "ACGT" else "N")
    return "".join(out)


def sigma(s, i, j, match, mismatch):
    return match if (s[i - 1], s[j - 1]) in PAIRS else -mismatch


# ---------------------------------------------------------------- the recurrence, cell by cell

def h_cells(s, max_span, match, mismatch, gap):
    """{(i, j): H} over the cells 1 <= i < j <= n with j - i + 1 <= max_span; every other cell counts as 0."""
    n, H = len(s), {}
    get = lambda i, j: H.get((i, j), 0)
    for i in range(n - 1, 0, -1):
        for j in range(i + 1, min(n, i + max_span - 1) + 1):
            H[(i, j)] = max(0, get(i + 1, j - 1) + sigma(s, i, j, match, mismatch), get(i + 1, j) - gap, get(i, j - 1) - gap)
    return H


def rows_of_cells(H, n, max_span):
    """(r, dstar), lists indexed 1..n (index 0 unused)."""
    r, dstar = [0] * (n + 1), [0] * (n + 1)
    for i in range(1, n + 1):
        for j in range(i + 1, min(n, i + max_span - 1) + 1):
            if H[(i, j)] > r[i]:
                r[i], dstar[i] = H[(i, j)], j - i
    return r, dstar


# ---------------------------------------------------------------- the same by levels

def h_levels(s, max_span, match, mismatch, gap):
    """L[d + 1, i - 1] = H(i, i + d) for d = -1 .. max_span - 1; columns past n - d stay 0."""
    n = len(s)
    code = np.frombuffer(s.encode(), dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    for x, y in PAIRS:
        comp[ord(x)] = ord(y)
    want = comp[code]                                       # the letter that pairs with base i (0 for N: equals nothing)
    L = np.zeros((max_span + 1, n + 2), dtype=np.int32)
    for d in range(1, min(max_span - 1, n - 1) + 1):
        m = n - d                                           # rows 1 .. n - d have a cell at this level
        sig = np.where(want[:m] == code[d:d + m], match, -mismatch).astype(np.int32)
        L[d + 1, :m] = np.maximum(np.maximum(L[d - 1, 1:m + 1] + sig, 0), np.maximum(L[d, 1:m + 1], L[d, :m]) - gap)
    return L


def rows_of_levels(L, n):
    r = np.concatenate(([0], L[:, :n].max(axis=0)))
    dstar = np.concatenate(([0], L[:, :n].argmax(axis=0) - 1))
    dstar[r == 0] = 0
    return [int(x) for x in r], [int(x) for x in dstar]


# ---------------------------------------------------------------- candidates, traceback, selection

def candidates(r, dstar, n, min_score):
    out = []
    for i in range(1, n + 1):
        if r[i] < min_score:
            continue
        if i > 1 and r[i - 1] > r[i] and dstar[i - 1] - dstar[i] in (1, 2):
            continue
        if i < n and r[i + 1] > r[i] and dstar[i] - dstar[i + 1] in (1, 2):
            continue
        out.append(i)
    return out


def traceback(get, s, i, j, match, mismatch, gap):
    """The unique alignment that ends at (i, j): a record without contig and name."""
    ops, a, b = [], i, j
    left_end = right_start = None
    while b > a and get(a, b) > 0:
        h, sg = get(a, b), sigma(s, a, b, match, mismatch)
        if h == get(a + 1, b - 1) + sg:
            ops.append("=" if sg > 0 else "X")
            left_end, right_start = a, b
            a, b = a + 1, b - 1
        elif h == get(a + 1, b) - gap:
            ops.append("L")
            left_end = a
            a += 1
        else:
            assert h == get(a, b - 1) - gap
            ops.append("R")
            right_start = b
            b -= 1
    ops = "".join(ops)
    return dict(score=get(i, j), left_start=i, left_end=left_end, right_start=right_start, right_end=j, matches=ops.count("="),
                mismatches=ops.count("X"), gaps=ops.count("L") + ops.count("R"), ops=ops)


def select(cands):
    """cands: records with `contig`.  Greedy by (score descending, contig, left_start, right_end); -> the accepted ones in output order."""
    taken, out = {}, []
    for rec in sorted(cands, key=lambda c: (-c["score"], c["contig"], c["left_start"], c["right_end"])):
        arms = [(rec["left_start"], rec["left_end"]), (rec["right_start"], rec["right_end"])]
        if any(s <= e2 and s2 <= e for s, e in arms for s2, e2 in taken.get(rec["contig"], [])):
            continue
        taken.setdefault(rec["contig"], []).extend(arms)
        out.append(rec)
    return sorted(out, key=lambda c: (c["contig"], c["left_start"], c["right_end"]))


def scan_contig(seq, engine="levels", **opts):
    """(get, r, dstar, candidate rows) of one contig."""
    o = dict(DEFAULTS, **opts)
    s, n = letters(seq), len(seq)
    if engine == "cells":
        H = h_cells(s, o["max_span"], o["match"], o["mismatch"], o["gap"])
        get = lambda i, j: H.get((i, j), 0)
        r, dstar = rows_of_cells(H, n, o["max_span"])
    else:
        L = h_levels(s, o["max_span"], o["match"], o["mismatch"], o["gap"])
        get = lambda i, j: int(L[j - i + 1, i - 1]) if 0 < j - i < o["max_span"] and j <= n else 0
        r, dstar = rows_of_levels(L, n)
    return get, r, dstar, candidates(r, dstar, n, o["min_score"])


def find(contigs, engine="levels", stats=None, **opts):
    """contigs: sequences (bytes / str) in file order -> the accepted repeats in output order, as records with `contig` (0-based) and `ops`."""
    o = dict(DEFAULTS, **opts)
    cands, above = [], 0
    for k, seq in enumerate(contigs):
        get, r, dstar, rows = scan_contig(seq, engine, **o)
        above += sum(1 for x in r[1:] if x >= o["min_score"])
        s = letters(seq)
        for i in rows:
            rec = traceback(get, s, i, i + dstar[i], o["match"], o["mismatch"], o["gap"])
            assert rec["score"] == r[i]
            rec["contig"] = k
            cands.append(rec)
    out = select(cands)
    if stats is not None:
        stats.update(rows_above=above, candidates=len(cands), accepted=len(out))
    return out


# ---------------------------------------------------------------- the files

def structure(ops):
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        out.append("%d%s" % (j - i, ops[i]))
        i = j
    return "".join(out)


def identity(rec):
    return 100.0 * rec["matches"] / (rec["matches"] + rec["mismatches"] + rec["gaps"])


def tsv_text(names, recs):
    lines = [TSV_HEADER]
    for k, r in enumerate(recs):
        lines.append("IR_%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%s\n" % (
            k + 1, names[r["contig"]], r["left_start"], r["right_end"], r["score"], r["left_start"], r["left_end"], r["right_start"], r["right_end"],
            r["right_start"] - r["left_end"] - 1, r["matches"], r["mismatches"], r["gaps"], identity(r), structure(r["ops"])))
    return "".join(lines)


def gff_text(names, recs):
    lines = ["##gff-version 3\n"]
    for k, r in enumerate(recs):
        lines.append("%s\tmir_prefer_amd\tinverted_repeat\t%d\t%d\t%d\t.\t.\tID=IR_%d;Left=%d..%d;Right=%d..%d;Loop=%d;Identity=%.2f\n" % (
            names[r["contig"]], r["left_start"], r["right_end"], r["score"], k + 1, r["left_start"], r["left_end"], r["right_start"], r["right_end"],
            r["right_start"] - r["left_end"] - 1, identity(r)))
    return "".join(lines)


def fasta_text(names, contigs, recs):
    lines = []
    for k, r in enumerate(recs):
        seq = contigs[r["contig"]]
        seq = seq if isinstance(seq, str) else bytes(seq).decode("latin-1")
        lines.append(">IR_%d %s:%d-%d score=%d\n%s\n" % (k + 1, names[r["contig"]], r["left_start"], r["right_end"], r["score"],
                                                        seq[r["left_start"] - 1:r["right_end"]].upper()))
    return "".join(lines)

"""Restatement of the search for natural antisense transcripts, twice, with no code shared between the two statements:

  find        plain Python: seeds by a dictionary, every band cell by the recurrence, the traceback, a quadratic selection, the three writers;
  find_numpy  seeds by comparing the k-mers of A and B' over all (x, y), H by anti-diagonals in numpy, the selection by sets of positions.

Both return (records, stats): the records in output order as dicts with the fields of MirpNatsRec and `cigar`, the stats under STAT_NAMES.
Positions are 1-based as in the definition.  Nothing here is fast, and nothing here is imported by the package."""
import numpy as np

MAX_LEN = 65535
DEFAULTS = dict(seed=16, band=64, max_occ=200, min_seeds=1, match=3, mismatch=4, gap=12, min_score=200, min_length=100)
STAT_NAMES = ("transcripts", "skipped", "bases", "kmers_ignored", "seed_hits", "candidates", "kept_candidates", "cells", "above", "traced", "regions",
              "pairs")
FIELDS = ("a", "b", "score", "a_start", "a_end", "a_len", "b_start", "b_end", "b_len", "matches", "mismatches", "gaps", "seeds", "bin")
TSV_HEADER = "name\ta\tb\tscore\ta_start\ta_end\ta_len\tb_start\tb_end\tb_len\tmatches\tmismatches\tgaps\tidentity\tseeds\tcigar\n"
PAIRS_HEADER = "a\tb\tregions\tcolumns\ta_covered\ta_cov\tb_covered\tb_cov\n"


# ---------------------------------------------------------------------------------------------------- plain Python

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


COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMPLEMENT[c] for c in reversed(s))


def sigma(A, Bp, i, j, match, mismatch):
    return match if A[i - 1] == Bp[j - 1] and A[i - 1] != "N" else -mismatch


def band_cells(A, Bp, q, W, match, mismatch, gap):
    """{(i, j): H} over the cells of the matrix with (q - 1) W <= i - j + m - 1 <= (q + 2) W - 1; every other cell counts as 0."""
    n, m, H = len(A), len(Bp), {}
    get = lambda i, j: H.get((i, j), 0)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            if (q - 1) * W <= i - j + m - 1 <= (q + 2) * W - 1:
                H[(i, j)] = max(0, get(i - 1, j - 1) + sigma(A, Bp, i, j, match, mismatch), get(i - 1, j) - gap, get(i, j - 1) - gap)
    return H


def band_cells_quick(A, Bp, q, W, match, mismatch, gap):
    """band_cells with the j loop cut to the band: the same dictionary."""
    n, m, H = len(A), len(Bp), {}
    get = lambda i, j: H.get((i, j), 0)
    for i in range(1, n + 1):
        for j in range(max(1, i + m - 1 - ((q + 2) * W - 1)), min(m, i + m - 1 - (q - 1) * W) + 1):
            H[(i, j)] = max(0, get(i - 1, j - 1) + sigma(A, Bp, i, j, match, mismatch), get(i - 1, j) - gap, get(i, j - 1) - gap)
    return H


def end_cell(H):
    """(score, i, j): the maximal cell with the smallest i, then the smallest j; (0, 0, 0) without a positive cell."""
    best = (0, 0, 0)
    for (i, j), h in H.items():
        if h > best[0] or (h == best[0] and h > 0 and (i, j) < (best[1], best[2])):
            best = (h, i, j)
    return best


def traceback(H, A, Bp, i, j, match, mismatch, gap):
    """-> (ops in A's 5'->3' order, i_start, j_start): diagonal first, then (i - 1, j) as I, then (i, j - 1) as D; stops at H = 0."""
    get = lambda i, j: H.get((i, j), 0)
    ops, first = [], (i, j)
    while get(i, j) > 0:
        first = (i, j)
        s = sigma(A, Bp, i, j, match, mismatch)
        if get(i, j) == get(i - 1, j - 1) + s:
            ops.append("=" if s > 0 else "X")
            i, j = i - 1, j - 1
        elif get(i, j) == get(i - 1, j) - gap:
            ops.append("I")
            i -= 1
        else:
            assert get(i, j) == get(i, j - 1) - gap
            ops.append("D")
            j -= 1
    return "".join(reversed(ops)), first[0], first[1]


def cigar(ops):
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append("%d%s" % (e - k, ops[k]))
        k = e
    return "".join(out)


def record(a, b, q, seeds, n, m, score, i_end, j_end, ops, i_start, j_start):
    return dict(a=a, b=b, score=score, a_start=i_start, a_end=i_end, a_len=n, b_start=m + 1 - j_end, b_end=m + 1 - j_start, b_len=m,
                matches=ops.count("="), mismatches=ops.count("X"), gaps=ops.count("I") + ops.count("D"), seeds=seeds, bin=q, cigar=cigar(ops))


def find(seqs, cells=band_cells_quick, **kw):
    o = dict(DEFAULTS)
    o.update(kw)
    k, W, M = o["seed"], o["band"], o["max_occ"]
    sc = (o["match"], o["mismatch"], o["gap"])
    kept = [s if 0 < len(s) <= MAX_LEN else "" for s in (letters(s) for s in seqs)]
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(transcripts=len(kept), skipped=sum(1 for s in kept if not s), bases=sum(len(s) for s in kept))
    where = {}          # k-mer -> [(transcript, x)], forward sense
    for t, s in enumerate(kept):
        for x in range(1, len(s) - k + 2):
            v = s[x - 1:x - 1 + k]
            if "N" not in v:
                where.setdefault(v, []).append((t, x))
    f = lambda v: len(where.get(v, ()))
    ignored = lambda v: f(v) > M or f(revcomp(v)) > M
    stats["kmers_ignored"] = sum(1 for v in where if ignored(v))
    seeds = {}
    for a, A in enumerate(kept):
        for x in range(1, len(A) - k + 2):
            v = A[x - 1:x - 1 + k]
            if "N" in v or ignored(v):
                continue
            for b, p in where.get(revcomp(v), ()):          # B'[y .. y + k - 1] = v where B[m + 2 - y - k .. m + 1 - y] = rc(v)
                if b > a:
                    m = len(kept[b])
                    y = m + 2 - p - k
                    key = (a, b, (x - y + m - 1) // W)
                    seeds[key] = seeds.get(key, 0) + 1
    stats["seed_hits"], stats["candidates"] = sum(seeds.values()), len(seeds)
    found = []
    for a, b, q in sorted(key for key, cnt in seeds.items() if cnt >= o["min_seeds"]):
        stats["kept_candidates"] += 1
        A, Bp = kept[a], revcomp(kept[b])
        H = cells(A, Bp, q, W, *sc)
        stats["cells"] += len(H)
        score, i, j = end_cell(H)
        if score < o["min_score"]:
            continue
        stats["above"] += 1
        stats["traced"] += 1
        ops, i0, j0 = traceback(H, A, Bp, i, j, *sc)
        if len(ops) >= o["min_length"]:
            found.append(record(a, b, q, seeds[(a, b, q)], len(A), len(Bp), score, i, j, ops, i0, j0))
    found.sort(key=lambda r: (r["a"], r["b"], -r["score"], r["a_start"], r["b_start"], r["bin"]))
    chosen = []
    for r in found:          # quadratic: against every accepted alignment of the pair
        clash = False
        for c in chosen:
            if (c["a"], c["b"]) == (r["a"], r["b"]) and r["a_start"] <= c["a_end"] and c["a_start"] <= r["a_end"] and \
                    r["b_start"] <= c["b_end"] and c["b_start"] <= r["b_end"]:
                clash = True
        if not clash:
            chosen.append(r)
    chosen.sort(key=lambda r: (r["a"], r["b"], r["a_start"], r["b_start"]))
    stats["regions"], stats["pairs"] = len(chosen), len({(r["a"], r["b"]) for r in chosen})
    return chosen, stats


def tsv_text(names, recs):
    out = [TSV_HEADER]
    for k, r in enumerate(recs):
        cols = r["matches"] + r["mismatches"] + r["gaps"]
        out.append("\t".join(["NAT_%d" % (k + 1), names[r["a"]], names[r["b"]]] + [str(r[f]) for f in FIELDS[2:12]] +
                             ["%.2f" % (100 * r["matches"] / cols), str(r["seeds"]), r["cigar"]]) + "\n")
    return "".join(out)


def pairs_text(names, recs):
    out, pairs = [PAIRS_HEADER], []
    for r in recs:
        if (r["a"], r["b"]) not in pairs:
            pairs.append((r["a"], r["b"]))
    for a, b in pairs:
        mine = [r for r in recs if (r["a"], r["b"]) == (a, b)]
        pa, pb = set(), set()
        for r in mine:
            pa.update(range(r["a_start"], r["a_end"] + 1))
            pb.update(range(r["b_start"], r["b_end"] + 1))
        out.append("%s\t%s\t%d\t%d\t%d\t%.2f\t%d\t%.2f\n" % (names[a], names[b], len(mine), sum(r["matches"] + r["mismatches"] + r["gaps"] for r in mine),
                                                            len(pa), 100 * len(pa) / mine[0]["a_len"], len(pb), 100 * len(pb) / mine[0]["b_len"]))
    return "".join(out)


def bed_text(names, recs):
    out = []
    for k, r in enumerate(recs):
        out.append("%s\t%d\t%d\tNAT_%d_a\t%d\t+\n" % (names[r["a"]], r["a_start"] - 1, r["a_end"], k + 1, r["score"]))
        out.append("%s\t%d\t%d\tNAT_%d_b\t%d\t+\n" % (names[r["b"]], r["b_start"] - 1, r["b_end"], k + 1, r["score"]))
    return "".join(out)


# ---------------------------------------------------------------------------------------------------- the independent statement (numpy)

_CODE = np.full(256, 4, dtype=np.int64)
for _ch, _v in zip(b"AaCcGgTtUu", (0, 0, 1, 1, 2, 2, 3, 3, 3, 3)):
    _CODE[_ch] = _v


def np_codes(seq):
    """bytes / str -> int64 codes A C G T = 0..3, everything else 4."""
    data = np.frombuffer(seq.encode("latin-1") if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    if (data >= 0x80).any():
        raise ValueError("a byte >= 0x80")
    return _CODE[data]


def np_rc(codes):
    return np.where(codes < 4, 3 - codes, 4)[::-1]


def np_kmers(codes, k):
    """value of the k-mer at every start (0-based), -1 where it holds an unknown letter."""
    if len(codes) < k:
        return np.zeros(0, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(codes, k)
    val = win @ (4 ** np.arange(k - 1, -1, -1, dtype=np.int64))
    return np.where((win < 4).all(axis=1), val, -1)


def np_band(ca, cb, q, W, match, mismatch, gap):
    """H of one band by anti-diagonals: Hs[t, d + 1] = H(i, j) with i + j = t and i - j + m - 1 = (q - 1) W + d, 0 outside the matrix.
    -> (Hs, delta, cells): delta[d] = i - j of column d + 1."""
    n, m, w3 = len(ca), len(cb), 3 * W
    delta = (q - 1) * W + np.arange(w3) - (m - 1)
    Hs = np.zeros((n + m + 1, w3 + 2), dtype=np.int32)
    pa, pb = np.concatenate(([8], ca)), np.concatenate(([9], np.where(cb < 4, cb, 5)))
    cells = 0
    # an anti-diagonal holds the columns of one parity; i rises and j falls along them, so the ends tell whether all of them lie in the matrix
    cols = [np.arange(p, w3, 2) for p in (0, 1)]
    diff = [delta[c] for c in cols]
    score = np.array([-mismatch, match])
    for t in range(2, n + m + 1):
        p = (t + int(delta[0])) & 1          # the columns c with t + delta[c] even
        c = cols[p]
        i = (t + diff[p]) >> 1
        j = t - i
        if i[0] < 1 or i[-1] > n or j[-1] < 1 or j[0] > m:
            ok = (i >= 1) & (i <= n) & (j >= 1) & (j <= m)
            c, i, j = c[ok], i[ok], j[ok]
            if len(c) == 0:
                continue
        cells += len(c)
        s = score[(pa[i] == pb[j]).view(np.int8)]
        Hs[t, c + 1] = np.maximum(np.maximum(0, Hs[t - 2, c + 1] + s), np.maximum(Hs[t - 1, c], Hs[t - 1, c + 2]) - gap)
    return Hs, delta, cells


def np_extend(ca, cb, q, W, match, mismatch, gap):
    """-> (score, i_end, j_end, ops, i_start, j_start, cells) of one band; ops None when the score is 0."""
    n, m = len(ca), len(cb)
    Hs, delta, cells = np_band(ca, cb, q, W, match, mismatch, gap)
    score = int(Hs.max())
    if score == 0:
        return 0, 0, 0, None, 0, 0, cells
    ts, cs = np.nonzero(Hs == score)
    ii = (ts + delta[cs - 1]) // 2
    jj = ts - ii
    pick = np.lexsort((jj, ii))[0]
    i, j = int(ii[pick]), int(jj[pick])
    i_end, j_end = i, j
    col = lambda i, j: i - j - int(delta[0]) + 1
    def h(i, j):
        c = col(i, j)
        return int(Hs[i + j, c]) if i >= 1 and j >= 1 and 1 <= c <= 3 * W else 0
    ops, first = [], (i, j)
    while h(i, j) > 0:
        first = (i, j)
        pair = ca[i - 1] == cb[j - 1] and ca[i - 1] < 4
        if h(i, j) == h(i - 1, j - 1) + (match if pair else -mismatch):
            ops.append("=" if pair else "X")
            i, j = i - 1, j - 1
        elif h(i, j) == h(i - 1, j) - gap:
            ops.append("I")
            i -= 1
        else:
            ops.append("D")
            j -= 1
    return score, i_end, j_end, "".join(ops[::-1]), first[0], first[1], cells


def np_cigar(ops):
    arr = np.frombuffer(ops.encode(), dtype=np.uint8)
    starts = np.concatenate(([0], np.nonzero(arr[1:] != arr[:-1])[0] + 1, [len(arr)]))
    return "".join("%d%s" % (e - s, chr(arr[s])) for s, e in zip(starts[:-1], starts[1:]))


def find_numpy(seqs, **kw):
    o = dict(DEFAULTS)
    o.update(kw)
    k, W, M = o["seed"], o["band"], o["max_occ"]
    codes = [np_codes(s) for s in seqs]
    codes = [c if 0 < len(c) <= MAX_LEN else c[:0] for c in codes]
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(transcripts=len(codes), skipped=sum(1 for c in codes if len(c) == 0), bases=int(sum(len(c) for c in codes)))
    fw = [np_kmers(c, k) for c in codes]
    bw = [np_kmers(np_rc(c), k) for c in codes]          # the k-mers of B'
    every = np.concatenate([v[v >= 0] for v in fw] + [np.zeros(0, dtype=np.int64)])
    values, counts = np.unique(every, return_counts=True)
    def f(v):
        at = np.searchsorted(values, v)
        at = np.minimum(at, max(len(values) - 1, 0))
        return np.where(values[at] == v, counts[at], 0) if len(values) else np.zeros(len(v), dtype=np.int64)
    def rc_value(v):
        out = np.zeros(len(v), dtype=np.int64)
        for _ in range(k):
            out = out * 4 + (3 - v % 4)
            v = v // 4
        return out
    drop = (counts > M) | (f(rc_value(values)) > M)
    stats["kmers_ignored"] = int(drop.sum())
    dropped = values[drop]
    found = []
    for a in range(len(codes)):
        for b in range(a + 1, len(codes)):
            if len(fw[a]) == 0 or len(bw[b]) == 0:
                continue
            xs, ys = np.nonzero((fw[a][:, None] == bw[b][None, :]) & (fw[a][:, None] >= 0))
            keep = ~np.isin(fw[a][xs], dropped)
            xs, ys = xs[keep], ys[keep]
            if len(xs) == 0:
                continue
            m, n = len(codes[b]), len(codes[a])
            bins, per_bin = np.unique((xs - ys + m - 1) // W, return_counts=True)
            stats["seed_hits"] += len(xs)
            stats["candidates"] += len(bins)
            cb = np_rc(codes[b])
            for q, cnt in zip(bins.tolist(), per_bin.tolist()):
                if cnt < o["min_seeds"]:
                    continue
                stats["kept_candidates"] += 1
                score, i_end, j_end, ops, i0, j0, cells = np_extend(codes[a], cb, q, W, o["match"], o["mismatch"], o["gap"])
                stats["cells"] += cells
                if score < o["min_score"]:
                    continue
                stats["above"] += 1
                stats["traced"] += 1
                if len(ops) < o["min_length"]:
                    continue
                found.append(dict(a=a, b=b, score=score, a_start=i0, a_end=i_end, a_len=n, b_start=m + 1 - j_end, b_end=m + 1 - j0, b_len=m,
                                  matches=ops.count("="), mismatches=ops.count("X"), gaps=len(ops) - ops.count("=") - ops.count("X"), seeds=cnt, bin=q,
                                  cigar=np_cigar(ops)))
    order = sorted(range(len(found)), key=lambda z: (found[z]["a"], found[z]["b"], -found[z]["score"], found[z]["a_start"], found[z]["b_start"],
                                                      found[z]["bin"]))
    taken = {}          # pair -> [(positions of A, positions of B)]
    chosen = []
    for z in order:
        r = found[z]
        pa, pb = set(range(r["a_start"], r["a_end"] + 1)), set(range(r["b_start"], r["b_end"] + 1))
        sets = taken.setdefault((r["a"], r["b"]), [])
        if any(pa & qa and pb & qb for qa, qb in sets):
            continue
        sets.append((pa, pb))
        chosen.append(r)
    chosen.sort(key=lambda r: (r["a"], r["b"], r["a_start"], r["b_start"]))
    stats["regions"], stats["pairs"] = len(chosen), len(taken)
    return chosen, stats

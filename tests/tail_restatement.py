"""Brute-force restatement of the 3' tail search of the read alignment (`align --tail`, DESIGN.md §12 "Tails") for the tests.  From the brute-force
end-to-end hits of tests/test_align_cpu.py it takes the reads left without a hit; for each of them it loops over every strand, every admissible
length m of the templated part, every contig and every offset, and applies the definition literally: the templated 5' part equals the genome
(an ambiguous genome base equals nothing, a read letter outside ACGT equals nothing), and the read base after it fails against the next genome base
(outside the contig, ambiguous, different, or not ACGT itself).  It uses no seeds and no index.  It writes the whole .sam and the .tails.tsv."""
import numpy as np

from tests.place_restatement import depth_of
from tests.test_align_cpu import LETTER, PG, brute_hits, load_reads, load_reference, revcomp, sam_bytes  # noqa: F401 (re-exported for the tests)


def tailed_hits(seqs, r, T, M):
    """Every tailed hit of the read r (a code array), whatever its stratum: [(tid, offset, strand, m)]."""
    L = len(r)
    out = []
    if L < M + 1:
        return out
    Tr = min(T, L - M)
    for strand, O in ((0, r), (1, revcomp(r))):
        for m in range(L - Tr, L):
            t = L - m
            templ = O[:m] if strand == 0 else O[t:]
            nxt = int(O[m]) if strand == 0 else int(O[t - 1])           # the read base next to the templated part, in genome direction
            if (templ > 3).any():
                continue
            for tid, s in enumerate(seqs):
                w = len(s) - m + 1
                if w <= 0:
                    continue
                ok = np.ones(w, dtype=bool)
                for i in range(m):
                    ok &= s[i:i + w] == templ[i]                        # an ambiguous base (code 4) equals no read base
                    if i % 8 == 7 and not ok.any():
                        break
                for o in np.nonzero(ok)[0]:
                    gp = int(o) + m if strand == 0 else int(o) - 1      # the next genome position in that direction
                    if 0 <= gp < len(s) and s[gp] < 4 and nxt < 4 and s[gp] == nxt:
                        continue                                        # the match goes on: not maximal
                    out.append((tid, int(o), strand, m))
    return out


def tail_order(tail):
    return (len(tail), ["ACGTN".index(ch) for ch in tail])


def tail_align(names, seqs, reads, hits, v, k, m=0, f=False, T=0, M=16, trim=False, pg=PG):
    """-> (the .sam bytes, the .tails.tsv bytes, stats, per read: None or {"t", "hits" (the whole best stratum), "suppressed"}).  hits: the
    brute-force end-to-end hits (any superset of those with <= v mismatches).  T = 0: exactly sam_bytes and no summary (None)."""
    nhead = 2 + len(names)
    out = sam_bytes(names, seqs, [], [], v, k, m, f, pg).split(b"\n")[:-1]
    assert len(out) == nhead
    st = dict(reads=len(reads), aligned=0, unaligned=0, suppressed=0, records=0, tailed=0, tail_suppressed=0)
    table, info, cache = {}, [], {}
    for (q, r), hs in zip(reads, hits):
        L = len(r)
        plain = [h for h in hs if h[3] <= v] if L > v else []
        if plain or not T:
            recs = sam_bytes(names, seqs, [(q, r)], [hs], v, k, m, f, pg).split(b"\n")[nhead:-1]
            out += recs
            best = min(h[3] for h in plain) if plain else None
            supp = bool(plain) and bool(m) and sum(h[3] == best for h in plain) > m
            st["suppressed" if supp else "aligned" if plain else "unaligned"] += 1
            st["records"] += len(recs)
            info.append(None)
            continue
        key = (r.tobytes(), T, M)
        if key not in cache:
            cache[key] = tailed_hits(seqs, r, T, M)
        th = cache[key]
        if not th:
            if not f:
                out.append(sam_bytes(names, seqs, [(q, r)], [[]], v, k, m, f, pg).split(b"\n")[nhead])
                st["records"] += 1
            st["unaligned"] += 1
            info.append(None)
            continue
        mb = max(h[3] for h in th)                                       # the best stratum: the shortest tail over both strands
        t = L - mb
        sel = sorted((h for h in th if h[3] == mb), key=lambda h: (h[0], h[1], h[2]))
        if m and len(sel) > m:
            if not f:
                seq = LETTER[r].tobytes().decode()
                out.append(("%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\tXM:i:%d" % (q, seq, "I" * L, m + 1)).encode())
                st["records"] += 1
            st["suppressed"] += 1
            st["tail_suppressed"] += 1
            info.append({"t": t, "hits": sel, "suppressed": True})
            continue
        tail = LETTER[r[L - t:]].tobytes().decode()                      # as sequenced, on both strands
        for tid, off, strand, _ in sel[:k]:
            O = r if strand == 0 else revcomp(r)
            assert (seqs[tid][off:off + mb] == (O[:mb] if strand == 0 else O[t:])).all()
            if trim:
                part, cigar = (O[:mb] if strand == 0 else O[t:]), "%dM" % mb
            else:
                part, cigar = O, ("%dM%dS" % (mb, t) if strand == 0 else "%dS%dM" % (t, mb))
            out.append(("%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tXA:i:0\tMD:Z:%d\tNM:i:0\tXT:Z:%s"
                        % (q, 16 * strand, names[tid], off + 1, cigar, LETTER[part].tobytes().decode(), "I" * len(part), mb, tail)).encode())
            st["records"] += 1
        st["aligned"] += 1
        st["tailed"] += 1
        row = table.setdefault(tail, [0, 0])
        row[0] += 1
        row[1] += depth_of(q)
        info.append({"t": t, "hits": sel, "suppressed": False})
    sam = b"".join(ln + b"\n" for ln in out)
    if not T:
        return sam, None, st, info
    tsv = "tail\tlength\treads\tdepth\n" + "".join("%s\t%d\t%d\t%d\n" % (tl, len(tl), table[tl][0], table[tl][1]) for tl in sorted(table, key=tail_order))
    return sam, tsv.encode(), st, info

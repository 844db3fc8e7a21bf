"""Brute-force restatement of the placement of multi-mapped reads (`align --place`, DESIGN.md §12 "Placement") for the tests: from the brute-force
hits of tests/test_align_cpu.py it takes each read's depth and best stratum, collects the unique reads of the file in a dict, sums a hit's weight in
a loop over the positions of its window, draws with Python integers and writes the whole .sam.  It uses no prefix sums and no binary searches."""
import re

from tests.test_align_cpu import brute_hits, load_reads, load_reference, parse_fasta, sam_bytes  # noqa: F401 (re-exported for the tests)

MASK = (1 << 64) - 1


def depth_of(qname):
    m = re.search(r"_x([0-9]+)$", qname)
    if not m:
        return 1
    d = int(m.group(1))
    return d if d <= 2 ** 32 - 1 else 1


def draw(codes, seed):
    """FNV-1a-64 over the code bytes, xor seed, splitmix64 finaliser."""
    x = 0xcbf29ce484222325
    for b in codes:
        x = ((x ^ int(b)) * 0x100000001b3) & MASK
    x ^= seed
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK
    x ^= x >> 31
    return x


def hits_of(seqs, reads, vmax):
    """brute_hits for every read, each distinct sequence searched once; a read with more than vmax bases outside ACGT has no hit (such a base
    mismatches everything), so it is not searched at all."""
    cache, out = {}, []
    for q, r in reads:
        key = r.tobytes()
        if key not in cache:
            cache[key] = brute_hits(seqs, [(q, r)], vmax)[0] if int((r > 3).sum()) <= vmax else []
        out.append(cache[key])
    return out


def best_stratum(r, hs, v):
    hs = [h for h in hs if h[3] <= v] if len(r) > v else []
    best = min((h[3] for h in hs), default=None)
    return sorted((h for h in hs if h[3] == best), key=lambda h: (h[0], h[1], h[2]))


def place(names, seqs, reads, hits, v, M, W, seed, mode, f=False):
    """-> (the .sam bytes, per read a dict: n, cls (None for unaligned / suppressed), idx, w (list or None), wt, r).  mode "u" or "r"."""
    sel = [best_stratum(r, hs, v) for (q, r), hs in zip(reads, hits)]
    u = {}
    for (q, r), s in zip(reads, sel):
        if len(s) == 1:
            key = (s[0][0], s[0][1] + 1)
            u[key] = u.get(key, 0) + depth_of(q)
    info, chosen = [], []
    for (q, r), s in zip(reads, sel):
        n, L = len(s), len(r)
        if n == 0 or n > M:
            info.append({"n": n, "cls": None, "suppressed": n > M})
            chosen.append([])
            continue
        if n == 1:
            info.append({"n": 1, "cls": "N", "idx": 0, "w": None, "wt": 0, "wc": 0})
            chosen.append([s[0]])
            continue
        x = draw(r, seed)
        w, wt, idx, cls, rr = None, 0, None, "R", None
        if mode == "u":
            w = []
            for t, off, strand, mm in s:
                q1, LN = off + 1, len(seqs[t])
                w.append(sum(u.get((t, p), 0) for p in range(max(1, q1 - W), min(LN, q1 + L - 1 + W) + 1)))
            wt = sum(w)
            assert wt < 2 ** 64
            if wt > 0:
                rr = x % wt
                run = 0
                for i, wi in enumerate(w):
                    run += wi
                    if run > rr:
                        idx = i
                        break
                cls = "U"
        if idx is None:
            idx = x % n
        info.append({"n": n, "cls": cls, "idx": idx, "w": w, "wt": wt, "wc": w[idx] if cls == "U" else 0, "r": rr})
        chosen.append([s[idx]])
    body = sam_bytes(names, seqs, reads, chosen, v, 1, 0, f).split(b"\n")[:-1]
    nhead = 2 + len(names)
    out, recs = body[:nhead], iter(body[nhead:])
    for i in info:
        if i["cls"] is None:
            if not f:
                ln = next(recs)
                assert ln.endswith(b"\tXM:i:0")
                out.append(ln[:-1] + b"%d" % (M + 1) if i["suppressed"] else ln)
            continue
        out.append(next(recs) + b"\tNH:i:%d\tXY:Z:%s\tXW:Z:%d/%d" % (i["n"], i["cls"].encode(), i["wc"], i["wt"]))
    assert next(recs, None) is None
    return b"".join(ln + b"\n" for ln in out), info

"""The definition of the signature verb as plain Python, for the CPU and GPU tests: the rule as a double loop over loci and
records with dict sums, the three output files as bytes, and a second, independent numpy statement of the scan (np.unique for U, V and the
placements, searchsorted for the join of the two strands and for the partner of a placement).

A locus is (name, type, contig, start, end, strand), 1-based inclusive; its strand is ignored.  Records are ALN_DTYPE arrays sorted by
(tid, pos).  A record is kept when min_len <= len <= max_len; its 5' end is pos on '+' and pos + len - 1 on '-'; it belongs to a locus of its
contig when the 5' end lies in [start, end]."""
import math

import numpy as np

from mir_prefer_amd.capi import DUPLEX_SITE_DTYPE, LOCUS_DTYPE, SIGNATURE_ROW_DTYPE

CHUNK = 4096
HEADER = (b"name\ttype\tcontig\tstart\tend\treads\tplus_reads\tminus_reads\tpeak_overlap\tpeak_reads\tpeak_z\tduplexes\tduplex_reads\t"
          b"duplex_fraction\tmajor_pos\tmajor_len\tmajor_plus\tmajor_minus\tmajor_rna\n")
DUPLEX_HEADER = b"name\tcontig\tpos\tlen\tplus_reads\tminus_reads\tpaired\tplus_rna\tminus_rna\n"
DEFAULTS = dict(min_len=20, max_len=25, max_overlap=30, overhang=2, min_reads=5)
_COMP = bytes.maketrans(b"ATGCU", b"UACGA")


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def locus_array(kept, names):
    arr = np.zeros(len(kept), LOCUS_DTYPE)
    for q, (_, _, contig, start, end, strand) in enumerate(kept):
        arr[q] = (names.index(contig), "+-.".index(strand), start, end)
    return arr


# ---------------------------------------------------------------------------------------------------- the rule, word by word
def scan_plain(alns, loci, **kw):
    """loci: LOCUS_DTYPE.  Every locus against every record -> a list of dicts {reads, plus, H (index k - 1), duplexes: [(p, L, d+, d-)] in
    (p, L) order}."""
    o = options(**kw)
    K, ov = o["max_overlap"], o["overhang"]
    out = []
    recs = alns.tolist()
    for tid, _, start, end in loci.tolist():
        U, V, pl = {}, {}, {}
        reads = plus = 0
        for rt, pos, depth, ln, rs, _ in recs:
            if rt != tid or ln < o["min_len"] or ln > o["max_len"]:
                continue
            f = pos + ln - 1 if rs else pos
            if f < start or f > end:
                continue
            reads += depth
            if rs:
                V[f] = V.get(f, 0) + depth
            else:
                plus += depth
                U[f] = U.get(f, 0) + depth
            pl[(pos, rs, ln)] = pl.get((pos, rs, ln), 0) + depth
        H = [sum(min(d, V.get(x + k - 1, 0)) for x, d in U.items() if x + k - 1 <= end) for k in range(1, K + 1)]
        dup = [(p, ln, d, pl[(p - ov, 1, ln)]) for (p, rs, ln), d in sorted(pl.items()) if rs == 0 and (p - ov, 1, ln) in pl]
        out.append({"reads": reads, "plus": plus, "H": H, "duplexes": dup})
    return out


def host_columns(reads, H, duplex_reads):
    """peak_overlap, peak_reads, peak_z and duplex_fraction as they are printed."""
    top = max(H)
    peak = H.index(top) + 1 if top else 0
    if top == min(H):
        z = "NA"
    else:
        vals = [float(h) for h in H]
        mean = sum(vals) / len(vals)
        z = "%.3f" % ((float(top) - mean) / math.sqrt(sum((v - mean) ** 2 for v in vals) / len(vals)))
    return peak, top, z, "%.4f" % (2.0 * duplex_reads / reads) if reads else "NA"


def _rna(seq, pos, strand, ln):
    s = bytes(seq[max(pos - 1, 0):max(pos - 1 + ln, 0)]).upper()
    return s.translate(_COMP)[::-1] if strand else s.replace(b"T", b"U")


def files_plain(alns, kept, names, seqs=None, **kw):
    """<base>.tsv, <base>.overlaps.tsv and <base>.duplexes.tsv as bytes from the double loop.  seqs: contig name -> bytes, or None."""
    o = options(**kw)
    sums = scan_plain(alns, locus_array(kept, names), **o)
    tsv = [HEADER]
    ovl = [b"name" + b"".join(b"\t%d" % k for k in range(1, o["max_overlap"] + 1)) + b"\n"]
    dup = [DUPLEX_HEADER]
    for (name, kind, contig, start, end, _), c in zip(kept, sums):
        paired = [min(dp, dm) for _, _, dp, dm in c["duplexes"]]
        peak, top, z, frac = host_columns(c["reads"], c["H"], sum(paired))
        if paired:
            p, ln, dp, dm = c["duplexes"][paired.index(max(paired))]                 # the first of the maximum in (p, L) order
            major = [b"%d" % p, b"%d" % ln, b"%d" % dp, b"%d" % dm, _rna(seqs[contig], p, 0, ln) if seqs is not None else b"*"]
        else:
            major = [b"0", b"0", b"0", b"0", b"*"]
        tsv.append(b"\t".join([name.encode(), kind.encode(), contig.encode(), b"%d" % start, b"%d" % end, b"%d" % c["reads"], b"%d" % c["plus"],
                               b"%d" % (c["reads"] - c["plus"]), b"%d" % peak, b"%d" % top, z.encode(), b"%d" % len(paired), b"%d" % sum(paired),
                               frac.encode()] + major) + b"\n")
        ovl.append(name.encode() + b"".join(b"\t%d" % h for h in c["H"]) + b"\n")
        for (p, ln, dp, dm), m in zip(c["duplexes"], paired):
            if m >= o["min_reads"]:
                rna = [_rna(seqs[contig], p, 0, ln), _rna(seqs[contig], p - o["overhang"], 1, ln)] if seqs is not None else [b"*", b"*"]
                dup.append(b"\t".join([name.encode(), contig.encode(), b"%d" % p, b"%d" % ln, b"%d" % dp, b"%d" % dm, b"%d" % m] + rna) + b"\n")
    return b"".join(tsv), b"".join(ovl), b"".join(dup)


# ---------------------------------------------------------------------------------------------------- the scan, vectorised
def _table(keys, depth):
    """np.unique of the keys with the exact int64 depth sum of every distinct one."""
    order = np.argsort(keys, kind="stable")
    uk, first = np.unique(keys[order], return_index=True)
    return uk, (np.add.reduceat(depth[order], first) if len(uk) else np.zeros(0, np.int64))


def scan_numpy(alns, loci, lens, **kw):
    """What capi.Context.signature_scan returns: SIGNATURE_ROW_DTYPE rows, H [loci, K], DUPLEX_SITE_DTYPE sites in (locus, pos, len) order and
    the stats.  U, V and the placement table are built once; a locus is a range of each."""
    o = options(**kw)
    K, ov = o["max_overlap"], o["overhang"]
    lens = np.asarray(lens, np.int64)
    loci = np.asarray(loci, LOCUS_DTYPE)
    nl = len(loci)
    tid = alns["tid"].astype(np.int64)
    pos = alns["pos"].astype(np.int64)
    ln = alns["len"].astype(np.int64)
    dep = alns["depth"].astype(np.int64)
    rs = alns["strand"].astype(np.int64)
    assert len(lens) < 1 << 14, "the placement keys below hold 14 bits of tid"
    kept = (ln >= o["min_len"]) & (ln <= o["max_len"])
    f = np.where(rs == 1, pos + ln - 1, pos)
    known = (tid >= 0) & (tid < len(lens))
    on = kept & known & (f >= 1) & (f <= (lens[np.clip(tid, 0, len(lens) - 1)] if len(lens) else 0))
    ukey, usum = _table(((tid << 32) + f)[on & (rs == 0)], dep[on & (rs == 0)])
    vkey, vsum = _table(((tid << 32) + f)[on & (rs == 1)], dep[on & (rs == 1)])
    pkey, psum = _table(((((tid << 32) + pos) << 17) | (rs << 16) | ln)[on], dep[on])
    lo = (loci["tid"].astype(np.int64) << 32) + loci["start"]
    hi = (loci["tid"].astype(np.int64) << 32) + loci["end"]
    rows = np.zeros(nl, SIGNATURE_ROW_DTYPE)
    H = np.zeros((nl, K), np.int64)
    cu, cv = np.concatenate([[0], np.cumsum(usum)]), np.concatenate([[0], np.cumsum(vsum)])
    ua, ub = np.searchsorted(ukey, lo, "left"), np.searchsorted(ukey, hi, "right")
    rows["plus_reads"] = cu[ub] - cu[ua]
    rows["reads"] = rows["plus_reads"] + cv[np.searchsorted(vkey, hi, "right")] - cv[np.searchsorted(vkey, lo, "left")]
    for k in range(1, K + 1):                                      # the join at overlap k: V at x + k - 1, and the x that still fit in the locus
        at = np.searchsorted(vkey, ukey + k - 1, "left")
        hit = at < len(vkey)
        hit[hit] = vkey[at[hit]] == ukey[hit] + k - 1
        m = np.zeros(len(ukey), np.int64)
        m[hit] = np.minimum(usum[hit], vsum[at[hit]])
        cm = np.concatenate([[0], np.cumsum(m)])
        fit = np.maximum(np.searchsorted(ukey, hi - (k - 1), "right"), ua)
        H[:, k - 1] = cm[fit] - cm[ua]
    # the duplexes of the whole table, in (tid, p, L) order: a '+' row whose partner (p - overhang, '-', L) exists
    plus = np.flatnonzero(((pkey >> 16) & 1) == 0)
    want = pkey[plus] - (ov << 17) + (1 << 16)
    at = np.searchsorted(pkey, want, "left")
    hit = at < len(pkey)
    hit[hit] = pkey[at[hit]] == want[hit]
    dk = pkey[plus[hit]] >> 17                                     # tid << 32 | p
    dl = pkey[plus[hit]] & 0xffff
    dp, dm = psum[plus[hit]], psum[at[hit]]
    paired = np.minimum(dp, dm)
    far = dk - ov + dl - 1                                         # the partner's 5' end
    da, db = np.searchsorted(dk, lo, "left"), np.searchsorted(dk, hi, "right")
    parts = []
    for q in range(nl):
        a, b = int(da[q]), int(db[q])
        if a == b:
            continue
        idx = a + np.flatnonzero(far[a:b] <= hi[q])
        if not len(idx):
            continue
        m = paired[idx]
        best = idx[int(np.argmax(m))]                              # the first of the maximum
        rows["duplexes"][q], rows["duplex_reads"][q] = len(idx), m.sum()
        rows["major_pos"][q], rows["major_len"][q], rows["major_plus"][q], rows["major_minus"][q] = dk[best] & 0xffffffff, dl[best], dp[best], dm[best]
        idx = idx[m >= o["min_reads"]]
        if len(idx):
            s = np.zeros(len(idx), DUPLEX_SITE_DTYPE)
            s["locus"], s["pos"], s["len"], s["plus_reads"], s["minus_reads"] = q, dk[idx] & 0xffffffff, dl[idx], dp[idx], dm[idx]
            parts.append(s)
    sites = np.concatenate(parts) if parts else np.zeros(0, DUPLEX_SITE_DTYPE)
    stats = {"records": len(alns), "kept": int(kept.sum()), "u_entries": len(ukey), "v_entries": len(vkey),
             "jobs": int(((ub - ua + CHUNK - 1) // CHUNK).sum()), "sites": len(sites)}
    if nl == 0:
        stats.update(kept=0, u_entries=0, v_entries=0)
    return rows, H, sites, stats

"""The definition of the reads-on-given-loci verb as plain Python, for the CPU and GPU tests: the three readers of a loci file,
the counting rule as a double loop over loci and records with dict sums, both output files as bytes, and a second, independent numpy statement
of the scan (candidate ranges by searchsorted over the sorted records, as the device path finds them, with np.unique placements).

A locus is (name, type, contig, start, end, strand), 1-based inclusive, strand "+", "-" or "."; records are ALN_DTYPE arrays sorted by
(tid, pos)."""
import re

import numpy as np

from mir_prefer_amd.capi import CLUSTER_DTYPE, LOCUS_DTYPE

HEADER = (b"name\ttype\tcontig\tstart\tend\tlocus_strand\treads\tplus_reads\tstrand\tdicer_call\tplacements\tmajor_pos\tmajor_strand\tmajor_len\t"
          b"major_reads\tmajor_rna\tshort\tr20\tr21\tr22\tr23\tr24\tlong\n")
PHAS_HEADER_FIELDS = 10
_COMP = bytes.maketrans(b"ATGCU", b"UACGA")
_INT = re.compile(r"[+-]?[0-9]+\Z")


class Refused(Exception):
    """A refused loci file: str(e) names the file and the 1-based line."""


def _accept(path, no, start, end, strand):
    if not (_INT.match(start) and _INT.match(end)):
        raise Refused("%s line %d: not whole numbers" % (path, no))
    start, end = int(start), int(end)
    if strand not in ("+", "-", ".", "?"):
        raise Refused("%s line %d: strand" % (path, no))
    return start, end, "." if strand == "?" else strand


def _finish(path, no, locus, seen, out):
    name, _, _, start, end, _ = locus
    if start < 1 or start > end or name in seen:
        raise Refused("%s line %d: interval or repeated name" % (path, no))
    seen.add(name)
    out.append(locus)


def read_gff(path, types=None):
    out, seen = [], set()
    text = open(path).read().split("\n")
    for no, line in enumerate(text, 1):
        line = line.rstrip("\r")
        if line.startswith("##FASTA"):
            break
        if line.startswith("#") or line.strip() == "":
            continue
        f = line.split("\t")
        if len(f) > 2 and types is not None and f[2] not in types:
            continue
        if len(f) < 9:
            raise Refused("%s line %d: columns" % (path, no))
        start, end, strand = _accept(path, no, f[3], f[4], f[6])
        ids = [a.strip()[3:] for a in f[8].split(";") if a.strip().startswith("ID=") and len(a.strip()) > 3]
        name = ids[0] if ids else "%s:%d-%d:%s" % (f[0], start, end, strand)
        _finish(path, no, (name, f[2], f[0], start, end, strand), seen, out)
    return out


def read_bed(path):
    out, seen = [], set()
    for no, line in enumerate(open(path).read().split("\n"), 1):
        line = line.rstrip("\r")
        if line.strip() == "" or line[0] == "#" or line[:5] == "track" or line[:7] == "browser":
            continue
        f = line.split("\t")
        if len(f) < 3:
            raise Refused("%s line %d: columns" % (path, no))
        start, end, strand = _accept(path, no, f[1], f[2], f[5] if len(f) >= 6 else ".")
        name = f[3] if len(f) >= 4 and f[3] not in (".", "") else "%s:%d-%d" % (f[0], start + 1, end)
        _finish(path, no, (name, ".", f[0], start + 1, end, strand), seen, out)
    return out


def read_phas(path):
    """The phasing output: a header line, then 10 tab-separated fields per line; contig, start and end are the first three."""
    out, seen = [], set()
    lines = open(path, "rb").read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, line in enumerate(lines[1:], 2):
        f = line.decode().split("\t")
        if len(f) != PHAS_HEADER_FIELDS:
            raise Refused("%s line %d: fields" % (path, no))
        start, end = int(f[1]), int(f[2])
        _finish(path, no, ("%s:%d-%d" % (f[0], start, end), "PHAS", f[0], start, end, "."), seen, out)
    return out


def keep(loci, names, lens):
    """-> (loci on contigs of the header, dropped count); Refused when one ends beyond its contig, none is left or there are more than 2^24."""
    ln = {}
    for n, l in zip(names, lens):
        if n not in ln:
            ln[n] = l
    kept = [l for l in loci if l[2] in ln]
    if any(l[4] > ln[l[2]] for l in kept) or not kept or len(kept) > 1 << 24:
        raise Refused("loci against the header")
    return kept, len(loci) - len(kept)


def locus_array(kept, names):
    arr = np.zeros(len(kept), LOCUS_DTYPE)
    for q, (_, _, contig, start, end, strand) in enumerate(kept):
        arr[q] = (names.index(contig), "+-.".index(strand), start, end)
    return arr


# ---------------------------------------------------------------------------------------------------- the rule, word by word
def scan_plain(alns, loci, lens, n_samples, stranded=False):
    """loci: LOCUS_DTYPE.  Every locus against every record -> a list of dicts {reads, plus, sizes, samples, pl} and the counted pairs."""
    out, pairs = [], 0
    recs = alns.tolist()
    for tid, strand, start, end in loci.tolist():
        c = {"reads": 0, "plus": 0, "sizes": [0] * 7, "samples": [0] * n_samples, "pl": {}}
        for rt, pos, depth, ln, rs, sample in recs:
            if rt != tid or rt < 0 or rt >= len(lens):
                continue
            s, e = max(pos, 1), min(pos + ln - 1, lens[rt])
            if s > e or e < start or s > end:
                continue
            if stranded and strand != 2 and strand != rs:
                continue
            assert sample < n_samples
            pairs += 1
            c["reads"] += depth
            c["plus"] += depth if rs == 0 else 0
            c["sizes"][0 if ln < 20 else 6 if ln > 24 else ln - 19] += depth
            c["samples"][sample] += depth
            c["pl"][(pos, rs, ln)] = c["pl"].get((pos, rs, ln), 0) + depth
        out.append(c)
    return out, pairs


def files_plain(alns, kept, names, lens, sample_names, stranded=False, seqs=None):
    """Both files as bytes from the double loop.  seqs: contig name -> bytes, or None."""
    sums, _ = scan_plain(alns, locus_array(kept, names), lens, len(sample_names), stranded)
    tsv = [HEADER]
    cnt = [b"name" + b"".join(b"\t" + s.encode() for s in sample_names) + b"\n"]
    for (name, kind, contig, start, end, strand), c in zip(kept, sums):
        reads, plus = c["reads"], c["plus"]
        if c["pl"]:
            sc = b"+" if 5 * plus >= 4 * reads else b"-" if 5 * plus <= reads else b"."
            d = c["sizes"][1:6]
            best = [20 + i for i in range(5) if d[i] == max(d)]
            dc = b"N" if 5 * sum(d) < 4 * reads or len(best) > 1 else str(best[0]).encode()
            (mp, ms, ml), mr = min(c["pl"].items(), key=lambda kv: (-kv[1], kv[0]))
            if seqs is None:
                rna = b"*"
            else:
                s = bytes(seqs[contig][max(mp - 1, 0):max(mp - 1 + ml, 0)]).upper()
                rna = s.translate(_COMP)[::-1] if ms else s.replace(b"T", b"U")
            major = [str(mp).encode(), b"+-"[ms:ms + 1], str(ml).encode(), str(mr).encode(), rna]
        else:
            sc, dc, major = b".", b"N", [b"0", b".", b"0", b"0", b"*"]
        tsv.append(b"\t".join([name.encode(), kind.encode(), contig.encode(), b"%d" % start, b"%d" % end, strand.encode(), b"%d" % reads, b"%d" % plus,
                               sc, dc, b"%d" % len(c["pl"])] + major + [b"%d" % x for x in c["sizes"]]) + b"\n")
        cnt.append(name.encode() + b"".join(b"\t%d" % x for x in c["samples"]) + b"\n")
    return b"".join(tsv), b"".join(cnt)


# ---------------------------------------------------------------------------------------------------- the scan, vectorised
def scan_numpy(alns, loci, lens, n_samples, stranded=False):
    """What capi.Context.locus_scan returns (CLUSTER_DTYPE rows, [loci, samples] counts, the stats without `jobs`), from the sorted records: the
    candidates of a locus are the records of its contig with pos in [start - M + 1, end], M the longest record."""
    lens = np.asarray(lens, np.int64)
    loci = np.asarray(loci, LOCUS_DTYPE)
    tid = alns["tid"].astype(np.int64)
    pos = alns["pos"].astype(np.int64)
    ln = alns["len"].astype(np.int64)
    dep = alns["depth"].astype(np.int64)
    rs = alns["strand"].astype(np.int64)
    sm = alns["sample"].astype(np.int64)
    known = (tid >= 0) & (tid < len(lens))
    last = np.minimum(pos + ln - 1, np.where(known, lens[np.clip(tid, 0, max(len(lens) - 1, 0))] if len(lens) else 0, 0))
    ok = known & (np.maximum(pos, 1) <= last)
    key = (tid << 32) + pos
    assert np.all(key[1:] >= key[:-1]), "the records are sorted by (tid, pos)"
    M = int(ln.max()) if len(alns) else 0
    cls = np.where(ln < 20, 0, np.where(ln > 24, 6, ln - 19))
    pk = (pos << 17) | (rs << 16) | ln
    out = np.zeros(len(loci), CLUSTER_DTYPE)
    out["tid"], out["start"], out["end"] = loci["tid"], loci["start"], loci["end"]
    sizes = np.zeros((len(loci), 7), np.int64)
    counts = np.zeros((len(loci), n_samples), np.int64)
    pairs = 0
    for q, (t, strand, start, end) in enumerate(loci.tolist()):
        a = int(np.searchsorted(key, (t << 32) + start - M + 1, "left"))
        b = int(np.searchsorted(key, (t << 32) + end, "right"))
        m = ok[a:b] & (last[a:b] >= start)
        if stranded and strand != 2:
            m &= rs[a:b] == strand
        idx = a + np.flatnonzero(m)
        if not len(idx):
            continue
        assert int(sm[idx].max()) < n_samples
        pairs += len(idx)
        d = dep[idx]
        out["reads"][q] = d.sum()
        out["plus_reads"][q] = d[rs[idx] == 0].sum()
        np.add.at(sizes[q], cls[idx], d)
        np.add.at(counts[q], sm[idx], d)
        up, inv = np.unique(pk[idx], return_inverse=True)
        psum = np.zeros(len(up), np.int64)
        np.add.at(psum, inv, d)
        best = int(np.argmax(psum))                        # the first of the maximum in (pos, strand, len) order
        out["placements"][q] = len(up)
        out["major_pos"][q], out["major_strand"][q], out["major_len"][q] = int(up[best]) >> 17, (int(up[best]) >> 16) & 1, int(up[best]) & 0xffff
        out["major_reads"][q] = psum[best]
    out["sizes"] = sizes
    return out, counts, {"records": len(alns), "loci": len(loci), "pairs": pairs, "max_len": M}

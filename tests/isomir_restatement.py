"""The definition of the isomiR counts (`isomirs`) as plain Python, for the tests: a SAM line parser, the GFF reader, the assignment as
a loop over the loci of a record's contig and strand with no sorted list and no search, dict sums, and the three files as bytes.  scan_numpy states
the same assignment a second way (for every pair of offsets in the order of the rule, the one locus with exactly those ends is looked up) for inputs
the dict version is too slow for; tests/test_isomirs_gpu.py checks the two against each other."""
import re

import numpy as np

DIGIT = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
_COMP_RNA = bytes.maketrans(b"ATGCU", b"UACGA")
N_SUMS = 11     # reads canonical shift5 trim3 ext3 tailed tail_u tail_a isomirs major_reads major


# ---------------------------------------------------------------------------------------------------- tails
def norm_tail(letters):
    return "".join(ch if ch in "ACGT" else "T" if ch == "U" else "N" for ch in letters.upper())


def tail_code(tail):
    """0 for no tail, else (5^t - 5) / 4 + 1 + sum digit_i 5^(t - 1 - i)."""
    t = len(tail)
    if t == 0:
        return 0
    return (5 ** t - 5) // 4 + 1 + sum(DIGIT[ch] * 5 ** (t - 1 - i) for i, ch in enumerate(tail))


_ALL_TAILS = {}


def tail_of_code(code):
    """The inverse of tail_code by enumeration (the codes are dense: 1 .. 488,280 for 1 .. 8 letters)."""
    if code == 0:
        return ""
    if not _ALL_TAILS:
        level = [""]
        for _ in range(8):
            level = [s + ch for s in level for ch in "ACGTN"]
            for s in level:
                _ALL_TAILS[tail_code(s)] = s
    return _ALL_TAILS[code]


# ---------------------------------------------------------------------------------------------------- SAM
def parse_record(fields, tid_of):
    """One alignment line as its tab-separated fields -> None (dropped: fewer than 10 fields or flag & 0x704), "cigar" / "long_tail" (skipped) or
    (tid, strand, p, m, depth, tail code); raises ValueError with the ingest's message."""
    if len(fields) < 10:
        return None
    if not re.fullmatch(r"[0-9]+", fields[1]):
        raise ValueError("SAM flag is not a number")
    flag = int(fields[1])
    if flag & 0x704:
        return None
    mt = re.match(r"^\S+_x([0-9]+)", fields[0])
    if not mt:
        raise ValueError("Read Id format is not right. Read id must be in \"samplename_rA_xN\" format.")
    depth = min(int(mt.group(1)), 0xffffffff)
    if fields[2] not in tid_of:
        raise ValueError("alignment refers to a sequence that is not in the @SQ header: " + fields[2])
    tid = tid_of[fields[2]]
    if not re.fullmatch(r"[0-9]+", fields[3]) or int(fields[3]) > 0x7ffffff0:
        raise ValueError("SAM position is not a number")
    p = int(fields[3])
    cigar, seq = fields[5], fields[9]
    if len(seq) > 65535:
        raise ValueError("read longer than 65535")
    if cigar == "*":
        raise ValueError("alignment without a CIGAR string")
    strand = 1 if flag & 16 else 0
    plain = re.fullmatch(r"([0-9]+)M", cigar)
    clip = re.fullmatch(r"([0-9]+)M([0-9]+)S", cigar) if strand == 0 else re.fullmatch(r"([0-9]+)S([0-9]+)M", cigar)
    if plain:
        m, t = int(plain.group(1)), 0
    elif clip:
        m, t = (int(clip.group(1)), int(clip.group(2))) if strand == 0 else (int(clip.group(2)), int(clip.group(1)))
        if t < 1:
            return "cigar"
    else:
        return "cigar"
    if not 1 <= m <= 65535:
        return "cigar"
    if seq != "*" and len(seq) != m + t:
        return "cigar"
    if t > 0:
        if seq == "*":
            return "cigar"
        if strand == 0:
            tail = norm_tail(seq[m:])
        else:
            tail = "".join(_COMP[ch] for ch in reversed(norm_tail(seq[:t])))
    else:
        tail = ""
        for opt in fields[11:]:
            if opt.startswith("XT:Z:"):
                tail = norm_tail(opt[5:])
                break
    if len(tail) > 8:
        return "long_tail"
    return tid, strand, p, m, depth, tail_code(tail)


def parse_sams(paths):
    """-> (contig names, lengths, sample names, [(tid, strand, p, m, depth, sample, tail code)] in (sample, file) order, {"cigar", "long_tail"})."""
    names, lens, samples, recs, skipped = [], [], [], [], {"cigar": 0, "long_tail": 0}
    tid_of = {}
    for fi, path in enumerate(paths):
        with open(path, "rb") as f:
            lines = f.read().decode("latin-1").split("\n")
        k = 0
        while k < len(lines) and lines[k].startswith("@"):
            if fi == 0 and lines[k].startswith("@SQ") and len(lines[k]) > 3:
                sn, ln = "", -1
                for part in lines[k].split("\t"):
                    if part.startswith("SN:"):
                        sn = part[3:]
                    if part.startswith("LN:"):
                        mt = re.match(r"\s*[+-]?[0-9]+", part[3:])
                        ln = int(mt.group(0)) if mt else 0
                sn = sn.rstrip("\r\n")
                if sn and ln >= 0:
                    names.append(sn)
                    lens.append(ln)
            k += 1
        if fi == 0:
            if not names:
                raise ValueError("Can not get the sequence length from the input SAM files. Make sure SAM files have headers.")
            for t, n in enumerate(names):
                tid_of.setdefault(n, t)
        first_id = lines[k].split("\t")[0] if k < len(lines) else ""
        parts = first_id.split("_")
        samples.append("_".join(parts[:-2]) if len(parts) >= 3 else "")
        for line in lines[k:]:
            if line.endswith("\r"):
                line = line[:-1]
            if not line or line.startswith("@"):
                continue
            got = parse_record(line.split("\t"), tid_of)
            if got is None:
                continue
            if isinstance(got, str):
                skipped[got] += 1
                continue
            tid, strand, p, m, depth, code = got
            recs.append((tid, strand, p, m, depth, fi, code))
    return names, lens, samples, recs, skipped


# ---------------------------------------------------------------------------------------------------- GFF
def read_gff(path):
    """The loci of a GFF3 file in file order: [(name, label, contig, start, end, strand)]; raises ValueError for a refused file."""
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("##FASTA"):
                break
            if line.startswith("#") or not line.strip():
                continue
            col = line.rstrip("\r\n").split("\t")
            if len(col) < 3 or col[2] != "miRNA":
                continue
            if len(col) < 9:
                raise ValueError("columns")
            attrs = [a.strip().partition("=") for a in col[8].split(";")]
            ids = [v for k, eq, v in attrs if eq and k == "ID"]
            labels = [v for k, eq, v in attrs if eq and k.lower() == "name"]
            if not ids or not ids[0]:
                raise ValueError("without an ID")
            start, end = int(col[3]), int(col[4])
            if start < 1:
                raise ValueError("before position 1")
            if start > end:
                raise ValueError("start behind its end")
            if col[6] not in "+-" or len(col[6]) != 1:
                raise ValueError("strand")
            out.append((ids[0], labels[0] if labels and labels[0] else ".", col[0], start, end, col[6]))
    if len(set(l[0] for l in out)) != len(out):
        raise ValueError("occurs twice")
    if len(set((l[2], l[5], l[3], l[4]) for l in out)) != len(out):
        raise ValueError("repeats the place")
    return out


def keep_loci(loci, names, lens):
    ln = {}
    for n, l in zip(names, lens):
        ln.setdefault(n, l)
    kept = [l for l in loci if l[2] in ln]
    for l in kept:
        if l[4] > ln[l[2]]:
            raise ValueError("beyond the end")
    if not kept:
        raise ValueError("no miRNA")
    return kept, len(loci) - len(kept)


# ---------------------------------------------------------------------------------------------------- assignment and sums
def offsets(strand, p, m, l_strand, start, end):
    """(d5, d3) of a record against a locus of the same strand."""
    if strand == 0:
        r5, r3, l5, l3, sg = p, p + m - 1, start, end, 1
    else:
        r5, r3, l5, l3, sg = p + m - 1, p, end, start, -1
    return sg * (r5 - l5), sg * (r3 - l3)


def assign(rec, loci_by_place, max5, max3):
    """rec = (tid, strand, p, m, ...); loci_by_place[(tid, strand)] = [(number, start, end)] in any order -> (number, d5, d3) or None."""
    best = None
    for num, start, end in loci_by_place.get((rec[0], rec[1]), ()):
        d5, d3 = offsets(rec[1], rec[2], rec[3], rec[1], start, end)
        if abs(d5) <= max5 and abs(d3) <= max3:
            cand = (abs(d5), abs(d3), num, d5, d3)
            if best is None or cand < best:
                best = cand
    return None if best is None else (best[2], best[3], best[4])


def scan_plain(recs, loci, max5, max3, n_samples):
    """recs: [(tid, strand, p, m, depth, sample, tail code)]; loci: [(tid, strand 0 / 1, start, end)] in file order.  -> {"isomirs": [(locus, d5, d3,
    tail code, reads)] in order, "sums": [[N_SUMS]] per locus, "locus_counts", "isomir_counts", "stats": (records, assigned, depth, isomirs)}."""
    by_place = {}
    for num, (tid, strand, start, end) in enumerate(loci):
        by_place.setdefault((tid, strand), []).append((num, start, end))
    iso, lc = {}, [[0] * n_samples for _ in loci]
    sums = [[0] * N_SUMS for _ in loci]
    assigned = depth_sum = 0
    for rec in recs:
        got = assign(rec, by_place, max5, max3)
        if got is None:
            continue
        num, d5, d3 = got
        depth, sample, code = rec[4], rec[5], rec[6]
        assigned += 1
        depth_sum += depth
        row = iso.setdefault((num, d5, d3, code), [0] * (n_samples + 1))
        row[0] += depth
        row[1 + sample] += depth
        lc[num][sample] += depth
        tail = tail_of_code(code)
        s = sums[num]
        s[0] += depth
        s[1] += depth if d5 == 0 and d3 == 0 and code == 0 else 0
        s[2] += depth if d5 != 0 else 0
        s[3] += depth if d3 < 0 else 0
        s[4] += depth if d3 > 0 else 0
        s[5] += depth if code != 0 else 0
        s[6] += depth if tail and set(tail) == {"T"} else 0
        s[7] += depth if tail and set(tail) == {"A"} else 0
    keys = sorted(iso)
    for s in sums:
        s[10] = -1
    for q, key in enumerate(keys):
        s = sums[key[0]]
        s[8] += 1
        if iso[key][0] > s[9] or s[10] < 0:
            s[9], s[10] = iso[key][0], q
    return {"isomirs": [key + (iso[key][0],) for key in keys], "sums": sums, "locus_counts": lc, "isomir_counts": [iso[key][1:] for key in keys],
            "stats": (len(recs), assigned, depth_sum, len(keys))}


def scan_numpy(alns, tails, loci, max5, max3, n_samples):
    """The same result from record arrays (ALN_DTYPE with pos = p and len = m; uint32 tail codes) and loci [(tid, strand, start, end)].  For every
    (|d5|, |d3|) in the order of the rule and every choice of signs, the locus whose ends are exactly the record's ends moved back by those offsets is
    looked up in a table keyed by (tid, strand, 5' end, span); among the hits of one (|d5|, |d3|) the smallest locus number wins."""
    L = np.array(loci, dtype=np.int64).reshape(-1, 4)
    l5 = np.where(L[:, 1] == 0, L[:, 2], L[:, 3])
    span = L[:, 3] - L[:, 2]
    ok = span < (1 << 17)                       # a longer locus admits no record: m <= 65535 and the offsets are at most 15
    lkey = ((L[:, 0] * 2 + L[:, 1]) << 48) | (l5 << 17) | np.where(ok, span, 0)
    order = np.argsort(lkey[ok], kind="stable")
    table, nums = lkey[ok][order], np.nonzero(ok)[0][order]
    tid, strand = alns["tid"].astype(np.int64), alns["strand"].astype(np.int64)
    p, m = alns["pos"].astype(np.int64), alns["len"].astype(np.int64)
    sg = 1 - 2 * strand
    r5 = np.where(strand == 0, p, p + m - 1)
    n = len(alns)
    best = np.full(n, -1, dtype=np.int64)
    bd5, bd3 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for a5 in range(max5 + 1):
        for a3 in range(max3 + 1):
            open_ = best < 0
            if not open_.any() or not len(table):
                continue
            cand = np.full(n, 1 << 62, dtype=np.int64)
            c5, c3 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            for d5 in sorted({a5, -a5}):
                for d3 in sorted({a3, -a3}):
                    # l5 = r5 - sg d5; the locus span = the record's span (m - 1) + d5 - d3
                    sp = m - 1 + d5 - d3
                    q5 = r5 - sg * d5
                    valid = open_ & (sp >= 0) & (sp < (1 << 17)) & (q5 >= 0)
                    key = ((tid * 2 + strand) << 48) | (np.where(valid, q5, 0) << 17) | np.where(valid, sp, 0)
                    at = np.minimum(np.searchsorted(table, key), len(table) - 1)
                    hit = valid & (table[at] == key)
                    better = hit & (nums[at] < cand)
                    cand[better] = nums[at][better]
                    c5[better], c3[better] = d5, d3
            took = cand < (1 << 62)
            best[took], bd5[took], bd3[took] = cand[took], c5[took], c3[took]
    sel = best >= 0
    depth = alns["depth"].astype(np.int64)[sel]
    sample = alns["sample"].astype(np.int64)[sel]
    code = np.asarray(tails).astype(np.int64)[sel]
    key = (best[sel] << 29) | ((bd5[sel] + 15) << 24) | ((bd3[sel] + 15) << 19) | code
    uniq, inv = np.unique(key, return_inverse=True)
    ni = len(uniq)
    reads = np.zeros(ni, dtype=np.int64)
    np.add.at(reads, inv, depth)
    ic = np.zeros((ni, n_samples), dtype=np.int64)
    np.add.at(ic, (inv, sample), depth)
    locus, d5, d3, tc = uniq >> 29, ((uniq >> 24) & 31) - 15, ((uniq >> 19) & 31) - 15, uniq & ((1 << 19) - 1)
    all_a = np.array([tail_code("A" * t) for t in range(1, 9)])
    all_t = np.array([tail_code("T" * t) for t in range(1, 9)])
    nl = len(loci)
    sums = np.zeros((nl, N_SUMS), dtype=np.int64)
    for col, mask in enumerate((np.ones(ni, bool), (d5 == 0) & (d3 == 0) & (tc == 0), d5 != 0, d3 < 0, d3 > 0, tc != 0, np.isin(tc, all_t),
                                np.isin(tc, all_a))):
        np.add.at(sums[:, col], locus[mask], reads[mask])
    np.add.at(sums[:, 8], locus, 1)
    sums[:, 10] = -1
    for q in range(ni):                         # isomiR order: the first of the largest
        if reads[q] > sums[locus[q], 9] or sums[locus[q], 10] < 0:
            sums[locus[q], 9], sums[locus[q], 10] = reads[q], q
    lc = np.zeros((nl, n_samples), dtype=np.int64)
    np.add.at(lc, (best[sel], sample), depth)
    return {"isomirs": list(zip(locus.tolist(), d5.tolist(), d3.tolist(), tc.tolist(), reads.tolist())), "sums": sums.tolist(),
            "locus_counts": lc.tolist(), "isomir_counts": ic.tolist(), "stats": (n, int(sel.sum()), int(depth.sum()), ni)}


# ---------------------------------------------------------------------------------------------------- files
def placement_rna(seq, pos, minus, length):
    s = bytes(seq[max(pos - 1, 0):max(pos - 1 + length, 0)]).upper()
    return s.translate(_COMP_RNA)[::-1] if minus else s.replace(b"T", b"U")


def files(result, kept, sample_names, seqs=None):
    """result: scan_plain's; kept: [(name, label, contig, start, end, strand)]; seqs: contig name -> bytes.  -> (tsv, counts, isomirs) bytes."""
    tsv = ["name\tlabel\tcontig\tstart\tend\tstrand\treads\tcanonical\tshift5\ttrim3\text3\ttailed\ttail_u\ttail_a\tisomirs\tmajor_d5\tmajor_d3\t"
           "major_tail\tmajor_reads\n"]
    cnt = ["name" + "".join("\t" + s for s in sample_names) + "\n"]
    iso = ["name\td5\td3\ttail\treads\tseq" + "".join("\t" + s for s in sample_names) + "\n"]
    for k, (name, label, contig, start, end, strand) in enumerate(kept):
        s = result["sums"][k]
        if s[8]:
            _, d5, d3, code, reads = result["isomirs"][s[10]]
            major = [str(d5), str(d3), tail_of_code(code) or ".", str(reads)]
        else:
            major = [".", ".", ".", "0"]
        tsv.append("\t".join([name, label, contig, str(start), str(end), strand] + [str(v) for v in s[:9]] + major) + "\n")
        cnt.append("\t".join([name] + [str(v) for v in result["locus_counts"][k]]) + "\n")
    for (num, d5, d3, code, reads), row in zip(result["isomirs"], result["isomir_counts"]):
        name, _, contig, start, end, strand = kept[num]
        tail = tail_of_code(code)
        seq = "*"
        if seqs is not None:
            if strand == "+":
                pos, length = start + d5, (end + d3) - (start + d5) + 1
            else:
                pos, length = start - d3, (end - d5) - (start - d3) + 1
            seq = placement_rna(seqs[contig], pos, strand == "-", length).decode("latin-1") + tail.lower().replace("t", "u")
        iso.append("\t".join([name, str(d5), str(d3), tail or ".", str(reads), seq] + [str(v) for v in row]) + "\n")
    return tuple("".join(x).encode("latin-1") for x in (tsv, cnt, iso))


def restate(gff_path, sam_paths, max5, max3, seqs=None):
    """The whole verb: -> ((tsv, counts, isomirs) bytes, stats dict as the command line reports them)."""
    names, lens, samples, recs, skipped = parse_sams(sam_paths)
    kept, dropped = keep_loci(read_gff(gff_path), names, lens)
    tid_of = {}
    for t, n in enumerate(names):
        tid_of.setdefault(n, t)
    loci = [(tid_of[l[2]], 0 if l[5] == "+" else 1, l[3], l[4]) for l in kept]
    res = scan_plain(recs, loci, max5, max3, len(sam_paths))
    st = {"records": res["stats"][0], "cigar": skipped["cigar"], "long_tail": skipped["long_tail"], "kept": len(kept), "dropped": dropped,
          "assigned": res["stats"][1], "depth": res["stats"][2], "isomirs": res["stats"][3]}
    return files(res, kept, samples, seqs), st, res

"""Host tests of the known-miRNA annotation (mir_prefer_amd.annotate): the tests' two restatements of the whole definition, a
plain-Python loop over (query, known, shift) and a numpy version vectorised over the known sequences and the shifts, each producing the bytes of
the hits file and of the summary file; hand-made cases that pin the shifts, the ties, the order, -k, the classes and the families; every option
error of the command line with its exit status, checked without opening a device; and the scan kernels' resource report (no scratch).  The GPU
tests (test_annotate_gpu.py) compare the device output with these restatements."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests.test_targets_cpu import MCODE, Refused, WS, parse_mirnas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mir-prefer_amd", "csrc")
HEADER = b"query\tknown\tfamily\tdistance\tmismatches\toffset5\toffset3\tquery_5to3\tpairs\tknown_5to3\n"
RNA = b"ACGUN"
RNA_A = np.frombuffer(RNA, dtype=np.uint8)
FAMILY = re.compile(rb"^(?:[A-Za-z0-9]+-)?(mir|let|lin)-?([0-9]+)", re.I)
CLASSES = (b"identical", b"isomir", b"homolog", b"novel")


# ---------------------------------------------------------------------------------------------------- inputs
def parse_known(datas, species=None):
    """The known FASTA files of §19 -> ([(id bytes, code array)], skipped): §14's rules, but a length outside 12..32 is skipped and counted, the id
    is the first word of the header, and --species keeps the ids that start with a listed prefix and '-'.  Refused carries (file index, record)."""
    out, skipped = [], 0
    for fi, data in enumerate(datas):
        rec = 0
        cur = None

        def finish():
            nonlocal skipped
            if cur is not None:
                if 12 <= len(cur[1]) <= 32:
                    out.append((cur[0], MCODE[np.frombuffer(bytes(cur[1]), dtype=np.uint8)]))
                else:
                    skipped += 1
        for line in re.split(rb"\r\n|\r|\n", data):
            if line.startswith(b">"):
                finish()
                cur = None
                rec += 1
                name = line[1:].strip(WS)
                if not name:
                    raise Refused((fi, rec), "name")
                if any(c >= 0x80 for c in name):
                    raise Refused((fi, rec), "byte")
                cur = (re.split(rb"[ \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f]", name)[0], bytearray())
            elif cur is not None:
                s = line.strip(WS)
                if any(c >= 0x80 for c in s):
                    raise Refused((fi, rec), "byte")
                cur[1].extend(s)
        finish()
    if species is not None:
        out = [(i, c) for i, c in out if any(i.startswith(p + b"-") for p in species)]
    if len(out) > 1 << 24:
        raise Refused((len(datas) - 1, 0), "count")
    return out, skipped


def family(w):
    m = FAMILY.match(w)
    if not m:
        return w
    kind = m.group(1).lower()
    return (b"miR" if kind == b"mir" else kind + b"-") + m.group(2)


def summary_name(hits_path):
    return (hits_path[:-4] if hits_path.endswith(".tsv") else hits_path) + ".summary.tsv"


# ---------------------------------------------------------------------------------------------------- restatement 1: plain loops
def best_shift_plain(q, k, E, M):
    """(distance, mismatches, |d|, d) of the reported shift of the pair, or None when no shift is admissible"""
    Lq, Lk = len(q), len(k)
    best = None
    for d in range(-E, E + 1):
        off3 = Lq + d - Lk
        if abs(off3) > E:
            continue
        mm = 0
        for j in range(max(d, 0), min(Lq + d, Lk)):
            a, b = q[j - d], k[j]
            if a > 3 or b > 3 or a != b:
                mm += 1
        if mm > M:
            continue
        cand = (mm + abs(d) + abs(off3), mm, abs(d), d)
        if best is None or cand < best:
            best = cand
    return best


def line_plain(qname, q, kid, k, dist, mm, d):
    Lq, Lk = len(q), len(k)
    a, p, b = bytearray(), bytearray(), bytearray()
    for x in range(min(d, 0), max(Lq + d, Lk)):
        hq, hk = 0 <= x - d < Lq, 0 <= x < Lk
        a.append(RNA[q[x - d]] if hq else ord("-"))
        b.append(RNA[k[x]] if hk else ord("-"))
        p.append(ord(".") if not (hq and hk) else ord("|") if q[x - d] == k[x] and q[x - d] < 4 else ord("x"))
    return b"%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (qname, kid, family(kid), dist, mm, d, Lq + d - Lk, bytes(a), bytes(p), bytes(b))


def _class(dist, mm):
    return 0 if dist == 0 else 1 if mm == 0 else 2


def restate_plain(queries, known, E=2, M=2, k=0):
    """-> (hits file bytes, summary file bytes, {hits, lines, classes [4]})"""
    text, summ = [HEADER], []
    counts = {"hits": 0, "lines": 0, "classes": [0, 0, 0, 0]}
    for qname, q in queries:
        hits = []
        for ki, (kid, kc) in enumerate(known):
            b = best_shift_plain(q, kc, E, M)
            if b is not None:
                hits.append((b[0], b[1], ki, b[3]))
        hits.sort()
        counts["hits"] += len(hits)
        if not hits:
            counts["classes"][3] += 1
            summ.append(b"%s\t%d\tnovel\t.\t.\t.\t.\t.\t.\t0\n" % (qname, len(q)))
            continue
        dist, mm, ki, d = hits[0]
        counts["classes"][_class(dist, mm)] += 1
        summ.append(b"%s\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (qname, len(q), CLASSES[_class(dist, mm)], known[ki][0], family(known[ki][0]), dist, mm,
                                                                    d, len(q) + d - len(known[ki][1]), len(hits)))
        for dist, mm, ki, d in hits[:k] if k else hits:
            text.append(line_plain(qname, q, known[ki][0], known[ki][1], dist, mm, d))
            counts["lines"] += 1
    return b"".join(text), b"".join(summ), counts


# ---------------------------------------------------------------------------------------------------- restatement 2: numpy over known x shifts
class KnownMatrix:
    """the known sequences as one [n, 32] code matrix (5 past the end) and their lengths"""
    def __init__(self, known):
        self.known = known
        self.n = len(known)
        self.codes = np.full((self.n, 32), 5, dtype=np.uint8)
        self.lens = np.zeros(self.n, dtype=np.int64)
        for i, (_, c) in enumerate(known):
            self.codes[i, :len(c)] = c
            self.lens[i] = len(c)


def hits_numpy(q, K, E, M):
    """-> arrays (distance, mismatches, known index, d) of the query's hits in output order"""
    Lq = len(q)
    if K.n == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z
    ds = np.arange(-E, E + 1)
    pos = np.arange(32)
    src = pos[None, :] - ds[:, None]                                  # [shift, known position] -> query position
    inq = (src >= 0) & (src < Lq)
    qrow = np.where(inq, np.asarray(q, dtype=np.uint8)[np.clip(src, 0, Lq - 1)], 6)          # 6 where the query is absent
    differ = (K.codes[None, :, :] != qrow[:, None, :]) | (K.codes[None, :, :] > 3) | (qrow[:, None, :] > 3)
    overlap = inq[:, None, :] & (pos[None, None, :] < K.lens[None, :, None])
    mm = (differ & overlap).sum(axis=2)                                # [shift, known]
    off3 = Lq + ds[:, None] - K.lens[None, :]
    ok = (np.abs(off3) <= E) & (mm <= M)
    dist = mm + np.abs(ds)[:, None] + np.abs(off3)
    code = ((dist * 8 + mm) * 8 + np.abs(ds)[:, None]) * 2 + (ds[:, None] > 0)
    code = np.where(ok, code, 1 << 40)
    pick = code.argmin(axis=0)
    ki = np.nonzero(ok.any(axis=0))[0]
    pk = pick[ki]
    hd, hm, d = dist[pk, ki], mm[pk, ki], ds[pk]
    order = np.lexsort((ki, hm, hd))
    return hd[order], hm[order], ki[order], d[order]


def line_numpy(qname, q, kid, k, dist, mm, d):
    Lq, Lk = len(q), len(k)
    c0 = min(d, 0)
    w = max(Lq + d, Lk) - c0
    a = np.full(w, ord("-"), dtype=np.uint8)
    b = a.copy()
    a[d - c0:d - c0 + Lq] = RNA_A[q]
    b[-c0:-c0 + Lk] = RNA_A[k]
    both = (a != ord("-")) & (b != ord("-"))
    p = np.where(both, np.where((a == b) & (a != ord("N")), ord("|"), ord("x")), ord(".")).astype(np.uint8)
    return b"\t".join([qname, kid, family(kid), b"%d" % dist, b"%d" % mm, b"%d" % d, b"%d" % (Lq + d - Lk), a.tobytes(), p.tobytes(), b.tobytes()]) + b"\n"


def blocks_numpy(queries, known, E=2, M=2, k=0, only=None, K=None):
    """per query (all, or the indices in `only`): (its lines of the hits file, its summary line, hits, class)"""
    K = K or KnownMatrix(known)
    out = []
    for qi in range(len(queries)) if only is None else only:
        qname, q = queries[qi]
        hd, hm, ki, d = hits_numpy(q, K, E, M)
        n = len(ki)
        if n == 0:
            out.append((b"", b"\t".join([qname, b"%d" % len(q), b"novel"] + [b"."] * 6 + [b"0"]) + b"\n", 0, 3))
            continue
        keep = min(n, k) if k else n
        lines = b"".join(line_numpy(qname, q, known[ki[i]][0], known[ki[i]][1], int(hd[i]), int(hm[i]), int(d[i])) for i in range(keep))
        cls = 0 if hd[0] == 0 else 1 if hm[0] == 0 else 2
        kid = known[ki[0]][0]
        summ = b"\t".join([qname, b"%d" % len(q), CLASSES[cls], kid, family(kid), b"%d" % hd[0], b"%d" % hm[0], b"%d" % d[0],
                           b"%d" % (len(q) + d[0] - len(known[ki[0]][1])), b"%d" % n]) + b"\n"
        out.append((lines, summ, n, cls))
    return out


def restate_numpy(queries, known, E=2, M=2, k=0):
    blocks = blocks_numpy(queries, known, E, M, k)
    counts = {"hits": sum(b[2] for b in blocks), "lines": sum(b[0].count(b"\n") for b in blocks), "classes": [sum(b[3] == c for b in blocks) for c in range(4)]}
    return HEADER + b"".join(b[0] for b in blocks), b"".join(b[1] for b in blocks), counts


def restate_files(query_path, known_paths, numpy=True, species=None, **kw):
    with open(query_path, "rb") as f:
        queries = parse_mirnas(f.read())
    datas = []
    for p in known_paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    known, skipped = parse_known(datas, species)
    hits, summ, counts = (restate_numpy if numpy else restate_plain)(queries, known, **kw)
    counts.update(queries=len(queries), known=len(known), skipped=skipped)
    return hits, summ, counts


# ---------------------------------------------------------------------------------------------------- seeded inputs
def random_seq(rng, L):
    return bytes(b"ACGU"[c] for c in rng.randint(0, 4, L))


def dress(rng, s, unknown=0.0, lower=0.0, t_for_u=0.5):
    s = bytearray(s)
    for i in range(len(s)):
        if s[i] == ord("U") and rng.rand() < t_for_u:
            s[i] = ord("T")
        if unknown and rng.rand() < unknown:
            s[i] = b"NRYX-."[rng.randint(0, 6)]
        if lower and rng.rand() < lower:
            s[i] = ord(chr(s[i]).lower())
    return bytes(s)


def variant(rng, s, max_shift=4, max_subs=6):
    """a relative of s: both ends moved by up to max_shift and up to max_subs substitutions, 12..32 nt"""
    s = bytearray(s)
    for _ in range(int(rng.randint(0, max_subs + 1))):
        s[int(rng.randint(0, len(s)))] = b"ACGU"[rng.randint(0, 4)]
    a, b = int(rng.randint(-max_shift, max_shift + 1)), int(rng.randint(-max_shift, max_shift + 1))
    s = random_seq(rng, a) + bytes(s) if a > 0 else bytes(s[-a:])
    s = s + random_seq(rng, b) if b > 0 else s[:len(s) + b]
    if len(s) > 32:
        s = s[:32]
    return s + random_seq(rng, max(0, 12 - len(s)))


KNOWN_IDS = ("ath-miR%d%s", "osa-MIR%d%s", "zma-miR%d%s-5p", "cel-let-%d%s", "cel-lin-%d%s", "miR%d%s", "novel_%d%s", "ath-mir-%d%s-3p", "hsa-let-%d%s")


def fasta_bytes(rng, records, ends=(b"\n",), width=None):
    out = bytearray()
    for name, seq in records:
        end = ends[int(rng.randint(0, len(ends)))]
        out += b">" + name + end
        w = width or (len(seq) + 1)
        for i in range(0, len(seq), w):
            out += seq[i:i + w] + end
    return bytes(out)


def make_mixed(seed, nq, nk, ends=(b"\n", b"\r\n", b"\r")):
    """-> (query FASTA bytes, [known FASTA bytes, known FASTA bytes]): every length 12..32 on both sides, unknown letters, T for U, lower case, all
    three line ends, multi-line sequences, known records of 11, 33, 40 and 0 nt (skipped), several species, duplicate names, and queries that are
    relatives of known sequences at every distance the options allow."""
    rng = np.random.RandomState(seed)
    base = [random_seq(rng, 12 + (i % 21)) for i in range(nk)]
    known = []
    for i, s in enumerate(base):
        if i % 7 == 3 and i >= 42:
            s = variant(rng, base[int(rng.randint(0, i))], 3, 2)          # families: known sequences close to each other
        name = KNOWN_IDS[i % len(KNOWN_IDS)].encode() % (150 + i // 3, b"abc"[i % 3:i % 3 + 1])
        if i % 4 == 0:
            name += b" MIMAT%07d Some species\tmiR%d" % (i, i)
        known.append((name, dress(rng, s, unknown=0.02 if i % 5 == 0 else 0.0, lower=0.3 if i % 6 == 0 else 0.0)))
    for L in (11, 33, 40, 0):
        known.insert(int(rng.randint(0, len(known))), (b"ath-miR%dx" % (9000 + L), random_seq(rng, L)))
    known.append(known[0])                                                # a duplicate record
    queries = []
    for i in range(nq):
        r = i % 4
        if r == 0:
            s = random_seq(rng, 12 + (i // 4) % 21)
        elif r == 1:
            s = MCODE_TO_RNA(known[int(rng.randint(0, len(known)))][1])
            if not 12 <= len(s) <= 32:
                s = random_seq(rng, 20)
        else:
            s = variant(rng, base[int(rng.randint(0, nk))], 4, 3 if r == 2 else 6)
        name = b"chr%d:%d-%d + miRNA-precursor_%d" % (i // 2 % 5, 100 * (i // 2), 100 * (i // 2) + 21, i // 2)          # names repeat in pairs
        queries.append((name, dress(rng, s, unknown=0.03 if i % 9 == 0 else 0.0, lower=0.5 if i % 10 == 0 else 0.0)))
    half = len(known) // 2
    return (fasta_bytes(rng, queries, ends, width=17), [fasta_bytes(rng, known[:half], ends, width=25), fasta_bytes(rng, known[half:], ends)])


def MCODE_TO_RNA(s):
    """the letters of a FASTA sequence as upper-case RNA, unknown letters as N"""
    return RNA_A[MCODE[np.frombuffer(bytes(s), dtype=np.uint8)]].tobytes()


# ---------------------------------------------------------------------------------------------------- the two restatements agree
@pytest.mark.parametrize("seed", [1, 2])
def test_numpy_restatement_agrees_with_the_plain_one(seed):
    qd, kds = make_mixed(seed, 84, 110)
    queries = parse_mirnas(qd)
    assert sorted({len(c) for _, c in queries}) == list(range(12, 33))
    assert any((c > 3).any() for _, c in queries) and len({n for n, _ in queries}) < len(queries)
    assert b"\r\n" in qd and re.search(rb"\r[^\n]", qd) and any(ch in qd for ch in b"acgut") and b"T" in qd
    total = 0
    for species in (None, [b"ath", b"cel"]):
        known, skipped = parse_known(kds, species)
        assert skipped == 4
        if species is None:
            assert len(known) == 111 and sorted({len(c) for _, c in known}) == list(range(12, 33))
        else:
            assert 0 < len(known) < 111 and all(i.startswith((b"ath-", b"cel-")) for i, _ in known)
        for E, M, k in ((2, 2, 0), (4, 6, 0), (0, 0, 0), (1, 3, 2), (4, 6, 1)):
            a = restate_plain(queries, known, E, M, k)
            b = restate_numpy(queries, known, E, M, k)
            assert a == b, (species, E, M, k)
            total += a[2]["hits"]
            assert a[1].count(b"\n") == len(queries) and a[0].count(b"\n") == 1 + a[2]["lines"]
            assert sum(a[2]["classes"]) == len(queries)
            if (E, M) == (4, 6) and species is None:
                assert all(c > 0 for c in a[2]["classes"]), a[2]
    assert total > 300


def test_known_fasta_rules_and_refusals():
    data = b"junk\n>ath-miR1a  MIMAT1\tx\nACGU\r\nacgu\rTTTT\n\n>short\n" + b"A" * 11 + b"\n>x\n" + b"G" * 32 + b"\n>long desc\n" + b"C" * 33 + b"\n>empty\n>x y\n" + b"U" * 12
    known, skipped = parse_known([data])
    assert [i for i, _ in known] == [b"ath-miR1a", b"x", b"x"] and skipped == 3
    assert list(known[0][1]) == [0, 1, 2, 3] * 2 + [3] * 4
    assert parse_known([data, data], [b"ath"])[0][1][0] == b"ath-miR1a" and len(parse_known([data, data], [b"ath"])[0]) == 2
    assert parse_known([data], [b"at"])[0] == [] and parse_known([data], [b"ATH"])[0] == []          # the whole prefix, case-sensitive
    assert parse_known([b""]) == ([], 0)
    for datas, rec, why in (([b">a\n" + b"A" * 12 + b"\n> \t\n" + b"A" * 12], (0, 2), "name"),
                            ([b">a\n" + b"A" * 12, b">a\n" + b"A" * 40 + b"\n>b\n" + b"A" * 11 + b"\xc3\xa9"], (1, 2), "byte"),
                            ([">é\n".encode() + b"A" * 12], (0, 1), "byte")):
        with pytest.raises(Refused) as e:
            parse_known(datas)
        assert (e.value.record, e.value.reason) == (rec, why), datas


# ---------------------------------------------------------------------------------------------------- hand-made cases
def _pair(q, k, **kw):
    """one query against one known sequence, both restatements -> the hit's fields, or None"""
    queries = parse_mirnas(b">q\n" + q + b"\n")
    known, _ = parse_known([b">ath-miR1\n" + k + b"\n"])
    got = restate_plain(queries, known, **kw)
    assert got == restate_numpy(queries, known, **kw)
    rows = got[0].split(b"\n")[1:-1]
    assert len(rows) <= 1
    return rows[0].split(b"\t") if rows else None


def test_the_table_of_the_definition():
    r = _pair(b"A" * 20, b"A" * 22)
    assert r[3:7] == [b"2", b"0", b"0", b"-2"]                 # d = 0, 1, 2 all give distance 2: the smallest |d|
    assert r[7:] == [b"A" * 20 + b"--", b"|" * 20 + b"..", b"A" * 22]
    r = _pair(b"UGACAGAAGAGAGUGAGCAC", b"UGACAGAAGAGAGUGAGCACA")
    assert r[3:7] == [b"1", b"0", b"0", b"-1"]
    r = _pair(b"GACAGAAGAGAGUGAGCACA", b"UGACAGAAGAGAGUGAGCAC")
    assert r[3:7] == [b"2", b"0", b"1", b"1"]
    assert r[7:] == [b"-GACAGAAGAGAGUGAGCACA", b"." + b"|" * 19 + b".", b"UGACAGAAGAGAGUGAGCAC-"]
    r = _pair(b"ACGU" * 5, b"CGUA" * 5)
    assert r[3:7] == [b"2", b"0", b"-1", b"-1"]
    assert r[7:] == [b"ACGU" * 5 + b"-", b"." + b"|" * 19 + b".", b"-" + b"CGUA" * 5]


def test_ties_between_shifts_prefer_the_negative_one():
    # a period-1 query inside a longer run: d = -1 and d = +1 give the same (distance, mismatches, |d|) only when the lengths allow both
    r = _pair(b"A" * 20, b"A" * 20, E=2, M=0)
    assert r[3:7] == [b"0", b"0", b"0", b"0"]
    r = _pair(b"CA" * 10, b"AC" * 10, E=1, M=0)                 # d = -1 and d = 1 both match all 19 overlap positions
    assert r[3:7] == [b"2", b"0", b"-1", b"-1"]


def test_letters_case_t_and_unknown():
    assert _pair(b"ugacagaagagagtgagcac", b"UGACAGAAGAGAGUGAGCAC")[3:7] == [b"0", b"0", b"0", b"0"]
    r = _pair(b"UGACAGAAGANAGUGAGCAC", b"UGACAGAAGANAGUGAGCAC")      # unknown against unknown is a mismatch
    assert r[3:5] == [b"1", b"1"] and r[8] == b"|" * 10 + b"x" + b"|" * 9 and r[7] == r[9] == b"UGACAGAAGANAGUGAGCAC"
    assert _pair(b"UGACAGAAGANAGUGAGCAC", b"UGACAGAAGANAGUGAGCAC", M=0) is None
    r = _pair(b"UGACAGAAGAXAGUGAGCAC", b"UGACAGAAGAGAGUGAGCAC")
    assert r[3:5] == [b"1", b"1"] and r[7] == b"UGACAGAAGANAGUGAGCAC"
    # an unknown letter in an overhang costs nothing beyond the overhang
    assert _pair(b"NUGACAGAAGAGAGUGAGCAC", b"UGACAGAAGAGAGUGAGCAC")[3:7] == [b"1", b"0", b"-1", b"0"]


def test_length_differences_beyond_e_give_no_hit():
    k = b"UGACAGAAGAGAGUGAGCACAUGC"
    assert _pair(k[:19], k, E=2) is None                       # 5 nt shorter: offset5 + offset3 cannot both stay within 2
    r = _pair(k[2:22], k, E=2)
    assert r[3:7] == [b"4", b"0", b"2", b"-2"]
    assert _pair(k[:20], k, E=2) is None and _pair(k[:20], k, E=4)[3:7] == [b"4", b"0", b"0", b"-4"]
    assert _pair(k, k[:20], E=4)[3:7] == [b"4", b"0", b"0", b"4"] and _pair(k, k[:20], E=3) is None
    assert _pair(b"A" * 12, b"A" * 32, E=4) is None
    assert _pair(k, k, E=0, M=0)[3:7] == [b"0", b"0", b"0", b"0"]


def test_mismatch_bound_and_shift_choice():
    k = b"UGACAGAAGAGAGUGAGCAC"
    q = bytearray(k)
    q[3], q[9], q[15] = ord("G"), ord("C"), ord("U")
    assert _pair(bytes(q), k, M=2) is None
    assert _pair(bytes(q), k, M=3)[3:5] == [b"3", b"3"]
    # M = 6 reaches what M = 5 does not
    for i in (1, 5, 18):
        q[i] = ord("C") if k[i] != ord("C") else ord("G")
    assert _pair(bytes(q), k, M=5) is None and _pair(bytes(q), k, M=6)[3:5] == [b"6", b"6"]


def test_order_max_hits_and_classes():
    q = b"UGACAGAAGAGAGUGAGCAC"
    one = bytearray(q)
    one[4] = ord("C")
    known = [(b"osa-miR9c", q + b"AU"), (b"ath-miR156b", bytes(one)), (b"far", b"C" * 20), (b"ath-miR156a-5p", q), (b"zma-MIR156x", q + b"A"), (b"dup", q),
             (b"ath-miR9", b"G" + q[:-1])]
    kd = b"".join(b">" + n + b"\n" + s + b"\n" for n, s in known)
    queries = parse_mirnas(b">q1 first\n" + q + b"\n>q2\n" + b"G" * 21 + b"\n>q3\n" + q[:-1] + b"\n>q4\n" + bytes(one[:-1]) + b"G\n")
    kn, _ = parse_known([kd])
    hits, summ, counts = restate_plain(queries, kn)
    assert (hits, summ, counts) == restate_numpy(queries, kn)
    rows = [r.split(b"\t") for r in hits.split(b"\n")[1:-1]]
    # per query: distance, then mismatches, then the known file order
    assert [(r[1], r[3], r[4]) for r in rows if r[0] == b"q1 first"] == [
        (b"ath-miR156a-5p", b"0", b"0"), (b"dup", b"0", b"0"), (b"zma-MIR156x", b"1", b"0"), (b"ath-miR156b", b"1", b"1"), (b"osa-miR9c", b"2", b"0"),
        (b"ath-miR9", b"2", b"0")]
    srows = [r.split(b"\t") for r in summ.split(b"\n")[:-1]]
    assert [r[0] for r in srows] == [b"q1 first", b"q2", b"q3", b"q4"]
    assert srows[0] == [b"q1 first", b"20", b"identical", b"ath-miR156a-5p", b"miR156", b"0", b"0", b"0", b"0", b"6"]
    assert srows[1] == [b"q2", b"21", b"novel"] + [b"."] * 6 + [b"0"]
    assert srows[2][2:4] == [b"isomir", b"ath-miR156a-5p"] and srows[2][5:9] == [b"1", b"0", b"0", b"-1"]
    assert srows[3][2:4] == [b"homolog", b"ath-miR156b"] and srows[3][5:7] == [b"1", b"1"]
    assert counts["classes"] == [1, 1, 1, 1]
    # -k keeps the first lines of every query and leaves the summary alone
    for k in (1, 2, 3):
        h2, s2, c2 = restate_plain(queries, kn, k=k)
        assert (h2, s2, c2) == restate_numpy(queries, kn, k=k)
        assert s2 == summ and c2["hits"] == counts["hits"]
        want = []
        seen = {}
        for r in hits.split(b"\n")[1:-1]:
            n = r.split(b"\t")[0]
            seen[n] = seen.get(n, 0) + 1
            if seen[n] <= k:
                want.append(r)
        assert h2 == HEADER + b"".join(r + b"\n" for r in want)
    # homolog needs a mismatch in the first line, not in any line
    assert srows[0][2] == b"identical" and any(r[4] != b"0" for r in rows if r[0] == b"q1 first")


def test_families():
    table = {b"ath-miR156a-5p": b"miR156", b"osa-MIR2118b": b"miR2118", b"cel-let-7-5p": b"let-7", b"novel_17": b"novel_17", b"miR156a": b"miR156",
             b"MIR166": b"miR166", b"let-7": b"let-7", b"lin-4": b"lin-4", b"cel-lin-4-3p": b"lin-4", b"hsa-mir-21": b"miR21", b"hsa-Let-7a": b"let-7",
             b"miR156a-5p": b"miR156", b"bantam": b"bantam", b"dme-bantam-3p": b"dme-bantam-3p", b"ath-miR": b"ath-miR", b"mir-": b"mir-",
             b"a-b-miR1": b"a-b-miR1", b"x_1-miR5": b"x_1-miR5", b"ath-miRf10": b"ath-miRf10", b"LIN28": b"lin-28", b"mir-let-7": b"let-7"}
    for w, f in table.items():
        assert family(w) == f, w


def test_summary_name():
    assert summary_name("a/x.fa.annot.tsv") == "a/x.fa.annot.summary.tsv" and summary_name("out") == "out.summary.tsv"
    from mir_prefer_amd import annotate
    assert annotate.summary_name("a/x.fa.annot.tsv") == "a/x.fa.annot.summary.tsv" and annotate.summary_name("out.txt") == "out.txt.summary.tsv"
    assert annotate.output_name("d/p_miRNA.mature.fa") == "d/p_miRNA.mature.fa.annot.tsv"


# ---------------------------------------------------------------------------------------------------- the command line, without a device
def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.annotate"] + args, cwd=str(cwd), capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    q, k = tmp_path / "q.fa", tmp_path / "k.fa"
    q.write_bytes(b">q\nUGACAGAAGAGAGUGAGCAC\n")
    k.write_bytes(b">ath-miR156a\nUGACAGAAGAGAGUGAGCAC\n")
    bad = [[], [str(q)], ["-m", "7", str(q), str(k)], ["-m", "-1", str(q), str(k)], ["-e", "5", str(q), str(k)], ["-e", "-1", str(q), str(k)],
           ["-e", "x", str(q), str(k)], ["-k", "-1", str(q), str(k)], ["-k", "1.5", str(q), str(k)], ["--species", "", str(q), str(k)],
           ["--species", "ath,,osa", str(q), str(k)], ["--species", "ath,", str(q), str(k)], ["--device", "-1", str(q), str(k)], ["-o", "", str(q), str(k)],
           ["-x", str(q), str(k)]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
        assert b"Error: " not in r.stderr
    assert not list(tmp_path.glob("*.tsv"))


def test_option_errors_do_not_import_the_binding():
    code = ("import sys\nfrom mir_prefer_amd import annotate\n"
            "for a in (['-m', '7', 'q', 'k'], ['-e', '5', 'q', 'k'], ['-k', '-1', 'q', 'k'], ['--species', '', 'q', 'k'], ['q']):\n"
            "    try:\n        annotate.main(a)\n    except SystemExit as e:\n        assert e.code == 2, (a, e.code)\n    else:\n        raise AssertionError(a)\n"
            "assert 'mir_prefer_amd.capi' not in sys.modules\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, timeout=120, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr.decode()


def test_missing_input_exits_255(tmp_path):
    (tmp_path / "q.fa").write_bytes(b">q\nUGACAGAAGAGAGUGAGCAC\n")
    r = run_cli([str(tmp_path / "q.fa"), str(tmp_path / "nope.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ") and "nope.fa" in r.stderr.decode()
    r = run_cli([str(tmp_path / "nope.fa"), str(tmp_path / "q.fa")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ")


def test_helpers_of_the_command_line(capsys):
    from mir_prefer_amd import annotate
    o, q, k, species, out, summ = annotate.parse_args(["-e", "3", "-m", "4", "-k", "5", "--species", "ath,osa", "q.fa", "a.fa", "b.fa"])
    assert (q, k, species, out, summ, o.max_offset, o.max_mismatches, o.max_hits) == ("q.fa", ["a.fa", "b.fa"], ["ath", "osa"], "q.fa.annot.tsv",
                                                                                     "q.fa.annot.summary.tsv", 3, 4, 5)
    o, q, k, species, out, summ = annotate.parse_args(["-o", "x.out", "q.fa", "a.fa"])
    assert (species, out, summ, o.max_offset, o.max_mismatches, o.max_hits) == ([], "x.out", "x.out.summary.tsv", 2, 2, 0)
    assert annotate.parse_species("ath") == ["ath"] and annotate.parse_species("a,") is None
    with pytest.raises(SystemExit) as e:
        annotate.parse_args(["-h"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for opt in ("--max-offset", "--max-mismatches", "--max-hits", "--species", "--output", "--device"):
        assert opt in text


# ---------------------------------------------------------------------------------------------------- the scan kernels' resources
def test_scan_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Wno-unused-result", "-Wno-missing-braces",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "annotate_kernels.hip"), "-o", str(tmp_path / "annotate_kernels.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    report = {}
    name = None
    for line in p.stdout.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            report[name][m.group(1).strip()] = int(m.group(2))
    scans = {k: v for k, v in report.items() if "an_scan_kernel" in k}
    assert len(scans) == 6, sorted(report)              # keys / counts / bins x lanes on either side
    for k, r in sorted(scans.items()):
        print(k, "VGPRs", r["VGPRs"], "SGPRs", r.get("TotalSGPRs"), "occupancy", r["Occupancy"], "scratch", r["ScratchSize"])
        assert r["ScratchSize"] == 0, (k, r)
    for k, r in report.items():
        assert r["ScratchSize"] == 0, (k, r)

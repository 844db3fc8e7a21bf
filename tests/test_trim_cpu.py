"""Host tests of the read trimming (mir_prefer_amd.trim): a plain-Python restatement that follows §13 line by line, a numpy
restatement vectorised over reads for large inputs, their self-checks (cutadapt's quality example, hand cases of the adapter rule, the per-mille
floor) and agreement on seeded random files, and the command line's argument errors, all without opening a device."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1024
NAME_LIMIT = 1 << 20
WS = frozenset([32, 9, 10, 11, 12, 13, 28, 29, 30, 31])
REASONS = ("line 1 does not start with '@'", "line 3 does not start with '+'", "the read is longer than 1,024 nt (not supported)",
           "the sequence and quality lengths differ", "the name is longer than 1,048,576 bytes (not supported)", "a quality byte is outside 33..126",
           "the file ends inside the record (a FASTQ record is 4 lines)")
STATS = ("reads", "quality_trimmed", "adapter", "untrimmed", "too_short", "too_long", "written")
ILLUMINA = "TGGAATTCTCGGGTGCCAAGG"


class Refused(Exception):
    """What the trim refuses: kind "ascii" (offset), "format", "quality", "reads", or "record" (1-based record, reason index into REASONS)."""

    def __init__(self, kind, record=None, reason=None, offset=None):
        super().__init__(kind, record, reason, offset)
        self.kind, self.record, self.reason, self.offset = kind, record, reason, offset


def strip(b):
    i, j = 0, len(b)
    while i < j and b[i] in WS:
        i += 1
    while j > i and b[j - 1] in WS:
        j -= 1
    return b[i:j]


def split_lines(data):
    """\\n, \\r\\n or a lone \\r ends a line; a line end at the very end of the data starts no new line."""
    if not data:
        return []
    lines = re.split(rb"\r\n|\r|\n", data)
    if data.endswith((b"\n", b"\r")):
        lines.pop()
    return lines


def name_of(header):
    w = header[1:]
    for i, c in enumerate(w):
        if c in WS:
            return w[:i]
    return w


def parse(data, q=0):
    """§13's input rules -> (is_fastq, [(name, read, qual or None)]), or Refused."""
    m = re.search(rb"[\x80-\xff]", data)
    if m:
        raise Refused("ascii", offset=m.start())
    if not data:
        return True, []
    if data[:1] not in (b"@", b">"):
        raise Refused("format")
    fq = data[:1] == b"@"
    if not fq and q > 0:
        raise Refused("quality")
    lines = split_lines(data)
    recs = []
    if fq:
        while lines and not strip(lines[-1]):
            lines.pop()
        n_rec, rem = divmod(len(lines), 4)
        if n_rec > 2 ** 31 - 1:
            raise Refused("reads")
        for r in range(n_rec):
            h, s, p, ql = lines[4 * r:4 * r + 4]
            seq, qual, name = strip(s), strip(ql), name_of(h)
            checks = (h[:1] != b"@", p[:1] != b"+", len(seq) > LIMIT, len(seq) != len(qual), len(name) > NAME_LIMIT,
                      any(c < 33 or c > 126 for c in qual))
            for k, bad in enumerate(checks):
                if bad:
                    raise Refused("record", record=r + 1, reason=k)
            recs.append((name, seq, qual))
        if rem:
            raise Refused("record", record=n_rec + 1, reason=6)
    else:
        for ln in lines:
            if ln[:1] == b">":
                recs.append([name_of(ln), []])
            else:
                recs[-1][1].append(strip(ln))
        if len(recs) > 2 ** 31 - 1:
            raise Refused("reads")
        recs = [(name, b"".join(parts), None) for name, parts in recs]
        for r, (name, read, _) in enumerate(recs):
            if len(read) > LIMIT:
                raise Refused("record", record=r + 1, reason=2)
            if len(name) > NAME_LIMIT:
                raise Refused("record", record=r + 1, reason=4)
    return fq, recs


def quality_cut(qual, cutoff):
    """The BWA / cutadapt 3' rule: the read keeps qual[:cut]."""
    s, best, cut = 0, 0, len(qual)
    for i in range(len(qual) - 1, -1, -1):
        s += cutoff - (qual[i] - 33)
        if s < 0:
            break
        if s > best:
            best, cut = s, i
    return cut


def adapter_pos(read, adapter, e_pm, overlap):
    """The first p whose overlap of length l = min(m, n - p) >= O has at most floor(E * l / 1000) mismatches; None without a match."""
    ad = adapter.upper()
    m, n = len(ad), len(read)
    for p in range(n + 1):
        ln = min(m, n - p)
        if ln < overlap:
            return None
        mism = 0
        for k in range(ln):
            c = read[p + k] & 0xdf if 97 <= read[p + k] <= 122 else read[p + k]
            if c not in b"ACGT" or c != ad[k]:
                mism += 1
        if mism <= e_pm * ln // 1000:
            return p
    return None


def restate_trim(data, adapter=b"", e_pm=100, overlap=3, q=0, min_len=18, max_len=0, discard=False):
    """Plain-Python restatement of §13: -> (output bytes, stats dict), or Refused."""
    adapter = adapter.encode() if isinstance(adapter, str) else adapter
    fq, recs = parse(data, q)
    st = dict.fromkeys(STATS, 0)
    out = []
    for name, read, qual in recs:
        st["reads"] += 1
        n = len(read)
        if fq and q > 0:
            cut = quality_cut(qual, q)
            if cut < n:
                st["quality_trimmed"] += 1
            read = read[:cut]
        found = False
        if adapter:
            p = adapter_pos(read, adapter, e_pm, overlap)
            if p is not None:
                found = True
                st["adapter"] += 1
                read = read[:p]
        if discard and not found:
            st["untrimmed"] += 1
        elif len(read) < min_len:
            st["too_short"] += 1
        elif max_len > 0 and len(read) > max_len:
            st["too_long"] += 1
        else:
            st["written"] += 1
            out.append(b">" + name + b"\n" + read + b"\n")
    return b"".join(out), st


# ---- numpy restatement (large inputs): the same rules, vectorised over reads

_WS_TABLE = np.zeros(256, bool)
_WS_TABLE[list(WS)] = True


def _ranges(lengths):
    """Concatenated aranges 0 .. lengths[i] - 1."""
    lengths = np.asarray(lengths, np.int64)
    tot = int(lengths.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    first = np.cumsum(lengths) - lengths
    return np.arange(tot, dtype=np.int64) - np.repeat(first, lengths)


def _np_lines(t):
    """Start and end (without the terminator) of every line of uint8 text t."""
    n = len(t)
    nl = t == 10
    cr = t == 13
    nxt = np.zeros(n, bool)
    nxt[:-1] = nl[1:]
    term = nl | (cr & ~nxt)                       # the byte that ends a line
    ends = np.flatnonzero(term)
    crlf = np.zeros(len(ends), bool)
    crlf[ends > 0] = cr[ends[ends > 0] - 1] & nl[ends[ends > 0]]
    last_open = len(ends) == 0 or ends[-1] != n - 1
    starts = np.concatenate([[0], ends + 1])[:len(ends) + (1 if last_open else 0)]
    stops = np.concatenate([ends - crlf, [n]])[:len(starts)]
    return starts.astype(np.int64), stops.astype(np.int64)


def _np_strip(t, b, e):
    b, e = b.copy(), e.copy()
    while True:
        m = (b < e) & _WS_TABLE[t[np.minimum(b, len(t) - 1)]]
        if not m.any():
            break
        b[m] += 1
    while True:
        m = (e > b) & _WS_TABLE[t[np.maximum(e - 1, 0)]]
        if not m.any():
            break
        e[m] -= 1
    return b, e


def restate_trim_numpy(data, adapter=b"", e_pm=100, overlap=3, q=0, min_len=18, max_len=0, discard=False):
    """The restatement for FASTQ input that parses cleanly (the refusals are the plain restatement's business), vectorised over reads."""
    adapter = adapter.encode() if isinstance(adapter, str) else adapter
    t = np.frombuffer(data, np.uint8)
    assert len(t) and t[0] == ord("@") and not (t >= 0x80).any()
    ls, le = _np_lines(t)
    keep = len(ls)
    while keep and not _np_strip(t, ls[keep - 1:keep], le[keep - 1:keep])[0][0] < _np_strip(t, ls[keep - 1:keep], le[keep - 1:keep])[1][0]:
        keep -= 1
    assert keep % 4 == 0
    R = keep // 4
    h = ls[0:keep:4]
    sb, se = _np_strip(t, ls[1:keep:4], le[1:keep:4])
    qb, qe = _np_strip(t, ls[3:keep:4], le[3:keep:4])
    assert (t[h] == ord("@")).all() and (t[ls[2:keep:4]] == ord("+")).all() and ((se - sb) == (qe - qb)).all() and (se - sb).max(initial=0) <= LIMIT
    wsp = np.flatnonzero(_WS_TABLE[t])
    k = np.searchsorted(wsp, h + 1)
    name_end = np.minimum(np.where(k < len(wsp), wsp[np.minimum(k, len(wsp) - 1)], len(t)), le[0:keep:4])
    nlen = name_end - (h + 1)
    n = (se - sb).astype(np.int64)
    W = int(n.max(initial=0)) + 1
    idx = np.minimum(sb[:, None] + np.arange(W)[None, :], len(t) - 1)
    inside = np.arange(W)[None, :] < n[:, None]
    seq = np.where(inside, t[idx], 0)
    L = n.copy()
    st = dict.fromkeys(STATS, 0)
    st["reads"] = R
    if q > 0:
        qual = np.where(inside, t[np.minimum(qb[:, None] + np.arange(W)[None, :], len(t) - 1)].astype(np.int64) - 33, 0)
        s = np.zeros(R, np.int64)
        best = np.zeros(R, np.int64)
        cut = n.copy()
        live = np.ones(R, bool)
        for i in range(W - 1, -1, -1):
            act = live & (i < n)
            s = np.where(act, s + q - qual[:, i], s)
            live &= ~(act & (s < 0))
            up = act & live & (s > best)
            best = np.where(up, s, best)
            cut = np.where(up, i, cut)
        st["quality_trimmed"] = int((cut < n).sum())
        L = cut
    found = np.zeros(R, bool)
    if adapter:
        ad = np.frombuffer(adapter.upper(), np.uint8)
        m = len(ad)
        upper = np.where((seq >= 97) & (seq <= 122), seq & 0xdf, seq)
        acgt = np.isin(upper, np.frombuffer(b"ACGT", np.uint8))
        upper = np.concatenate([upper, np.zeros((R, m), upper.dtype)], axis=1)
        acgt = np.concatenate([acgt, np.zeros((R, m), bool)], axis=1)
        pos = L.copy()
        for p in range(W):
            ln = np.minimum(m, L - p)
            act = ~found & (ln >= overlap)
            if not act.any():
                break
            rows = np.flatnonzero(act)
            mis = (upper[rows, p:p + m] != ad[None, :]) | ~acgt[rows, p:p + m]
            mis &= np.arange(m)[None, :] < ln[rows, None]
            hit = mis.sum(axis=1) <= (e_pm * ln[rows]) // 1000
            found[rows[hit]] = True
            pos[rows[hit]] = p
        st["adapter"] = int(found.sum())
        L = np.where(found, pos, L)
    untr = ~found if discard else np.zeros(R, bool)
    short = ~untr & (L < min_len)
    long_ = ~untr & ~short & (max_len > 0) & (L > max_len)
    wr = ~untr & ~short & ~long_
    st["untrimmed"], st["too_short"], st["too_long"], st["written"] = int(untr.sum()), int(short.sum()), int(long_.sum()), int(wr.sum())
    w = np.flatnonzero(wr)
    nl, fl = nlen[w], L[w]
    size = nl + fl + 3
    off = np.cumsum(size) - size
    out = np.empty(int(size.sum()), np.uint8)
    out[off] = ord(">")
    out[np.repeat(off + 1, nl) + _ranges(nl)] = t[np.repeat(h[w] + 1, nl) + _ranges(nl)]
    out[off + 1 + nl] = 10
    out[np.repeat(off + 2 + nl, fl) + _ranges(fl)] = t[np.repeat(sb[w], fl) + _ranges(fl)]
    out[off + size - 1] = 10
    return out.tobytes(), st


# ---- seeded inputs shared with the GPU tests

def fastq_record(name, seq, qual, eol=b"\n"):
    return b"@" + name + eol + seq + eol + b"+" + eol + qual + eol


def make_reads(rng, n, adapter=ILLUMINA, err=0.05, lo=0, hi=40, tail=(0, 30), dimers=0.05, alphabet=b"ACGTacgtN"):
    """Random inserts with planted adapter prefixes (some with errors), dimers, N and lower case: [(name, seq, qual)]."""
    ab = np.frombuffer(alphabet, np.uint8)
    ad = adapter.encode() if isinstance(adapter, str) else adapter
    out = []
    for i in range(n):
        ins = ab[rng.randint(0, len(ab), size=rng.randint(lo, hi + 1))].tobytes()
        if rng.rand() < dimers:
            ins = b""
        a = bytearray(ad[:rng.randint(0, len(ad) + 1)])
        for k in range(len(a)):
            if rng.rand() < err:
                a[k] = b"ACGTN"[rng.randint(0, 5)]
        tl = b"".join(b"ACGT"[x:x + 1] for x in rng.randint(0, 4, size=rng.randint(tail[0], tail[1] + 1)))
        seq = ins + bytes(a) + (tl if len(a) == len(ad) else b"")
        qual = bytes(np.clip(41 - np.arange(len(seq)) // 3 + rng.randint(-6, 7, size=len(seq)), 0, 41).astype(np.uint8) + 33)
        out.append((b"r%d" % i + (b" extra words" if i % 3 == 0 else b""), seq, qual))
    return out


def to_fastq(reads, eol=b"\n", final_eol=True):
    data = b"".join(fastq_record(n, s, q, eol) for n, s, q in reads)
    return data if final_eol else data[:-len(eol)]


def to_fasta(reads, eol=b"\n", width=0):
    parts = []
    for n, s, _ in reads:
        parts.append(b">" + n + eol)
        if width and len(s) > width:
            parts.extend(s[i:i + width] + eol for i in range(0, len(s), width))
        else:
            parts.append(s + eol)
    return b"".join(parts)


# ---- self-checks of the restatements

def test_cutadapt_quality_example():
    qual = bytes(x + 33 for x in (42, 40, 26, 27, 8, 7, 11, 4, 2, 3))
    assert quality_cut(qual, 10) == 4
    out, st = restate_trim(fastq_record(b"x", b"ACGTACGTAC", qual), q=10, min_len=0)
    assert out == b">x\nACGT\n" and st["quality_trimmed"] == 1


def test_adapter_rule_hand_cases():
    ad = b"TGGAATTC"
    assert adapter_pos(b"TGGAATTCAAAA", ad, 0, 3) == 0                 # dimer
    assert adapter_pos(b"ACGTACGTTGG", ad, 0, 3) == 8                  # partial overlap at the 3' end
    assert adapter_pos(b"ACGTACGTTG", ad, 0, 3) is None                # l = 2 < O
    assert adapter_pos(b"ACGTACGTTG", ad, 0, 2) == 8
    assert adapter_pos(b"acgttggaattc", ad, 0, 3) == 4                 # lower case matches
    assert adapter_pos(b"ACGTTGGANTTC", ad, 0, 3) is None              # N is a mismatch, never a wildcard
    assert adapter_pos(b"ACGTTGGANTTC", ad, 125, 3) == 4               # floor(0.125 * 8) = 1 error
    assert adapter_pos(b"ACGTTGGAATTA", ad, 100, 3) is None            # floor(0.1 * 8) = 0 errors
    assert adapter_pos(b"ACGTTGGAATTA", ad, 125, 3) == 4
    assert adapter_pos(b"ACGA", ad, 0, 1) is None
    assert adapter_pos(b"ACGT", ad, 0, 1) == 3                         # a one-base overlap at O = 1
    assert adapter_pos(b"ACGTT", ad, 0, 1) == 4


def test_per_mille_floor_is_exact():
    ad = b"A" * 100
    read = b"C" * 29 + b"A" * 71
    assert int(0.29 * 100) == 28                                      # the floating-point floor that §13 avoids
    assert adapter_pos(read, ad, 290, 100) == 0                       # 29 errors allowed at l = 100
    assert adapter_pos(b"C" * 30 + b"A" * 70, ad, 290, 100) is None


def test_fasta_multiline_and_names():
    data = b">a b\nACG\n TT \n\n>\nAC\n>c\tx\n"
    out, st = restate_trim(data, min_len=0)
    assert out == b">a\nACGTT\n>\nAC\n>c\n\n" and st["reads"] == 3 and st["written"] == 3


def test_refusals_of_the_restatement():
    good = fastq_record(b"a", b"ACGT", b"IIII")
    cases = [(good + b"@b\nAC\n+\n", ("record", 2, 6)), (good + b"Xb\nAC\n+\nII\n", ("record", 2, 0)), (good + b"@b\nAC\n-\nII\n", ("record", 2, 1)),
             (good + b"@b\n" + b"A" * 1025 + b"\n+\n" + b"I" * 1025 + b"\n", ("record", 2, 2)), (good + b"@b\nAC\n+\nI\n", ("record", 2, 3)),
             (good + b"@b\nAC\n+\nI \n", ("record", 2, 3)), (good + b"@b\nAC\n+\nI\x7f\n", ("record", 2, 5)),
             (b"ACGT\n", ("format", None, None)), (b">a\n" + b"A" * 1025, ("record", 1, 2))]
    for data, want in cases:
        with pytest.raises(Refused) as e:
            restate_trim(data)
        assert (e.value.kind, e.value.record, e.value.reason) == want, data[:40]
    with pytest.raises(Refused) as e:
        restate_trim(good + b"\xc3\xa9")
    assert e.value.offset == len(good)
    with pytest.raises(Refused) as e:
        restate_trim(b">a\nACGT\n", q=20)
    assert e.value.kind == "quality"
    assert restate_trim(good + b"\n \r\n\t\n", min_len=0)[0] == b">a\nACGT\n"     # trailing blank lines are ignored
    assert restate_trim(b"", min_len=0) == (b"", dict.fromkeys(STATS, 0))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_numpy_restatement_agrees_with_the_plain_one(seed):
    rng = np.random.RandomState(seed)
    reads = make_reads(rng, 3000)
    eol = (b"\n", b"\r\n", b"\r")[seed % 3]
    data = to_fastq(reads, eol, final_eol=seed != 2)
    for kw in (dict(adapter=ILLUMINA), dict(adapter=ILLUMINA, e_pm=0, overlap=1, q=20, min_len=5, max_len=30),
               dict(adapter="TGG", e_pm=250, discard=True, min_len=0), dict(q=15, min_len=10), dict(adapter="A" * 64, overlap=64, e_pm=290)):
        assert restate_trim_numpy(data, **kw) == restate_trim(data, **kw), kw


# ---- the command line's argument errors (no device is opened)

def run_cli(args, cwd, timeout=120):
    return subprocess.run([sys.executable, "-m", "mir_prefer_amd.trim"] + args, cwd=cwd, capture_output=True, timeout=timeout,
                          env=dict(os.environ, PYTHONPATH=ROOT))


def test_option_errors_exit_2_before_a_device(tmp_path):
    fq = tmp_path / "a.fastq"
    fq.write_bytes(fastq_record(b"a", b"ACGT", b"IIII"))
    fa = tmp_path / "a.fa"
    fa.write_bytes(b">a\nACGT\n")
    bad = [[], ["-a", "ACGU", str(fq)], ["-a", "A" * 65, str(fq)], ["-a", "", str(fq)], ["-e", "1", str(fq)], ["-e", "0.1234", str(fq)],
           ["-e", "1e-1", str(fq)], ["-e", "-0.1", str(fq)], ["-a", "ACG", "-O", "4", str(fq)], ["-a", "ACG", "-O", "0", str(fq)], ["-O", "2", str(fq)],
           ["-q", "94", str(fq)], ["-q", "-1", str(fq)], ["-m", "-1", str(fq)], ["-m", "20", "-M", "19", str(fq)], ["-M", "-2", str(fq)],
           ["--discard-untrimmed", str(fq)], ["--device", "-1", str(fq)], ["-q", "20", str(fa)], ["-x", str(fq)], ["-q", "x", str(fq)]]
    for args in bad:
        r = run_cli(args, tmp_path)
        assert r.returncode == 2, (args, r.stderr.decode())
    assert not list(tmp_path.glob("*.trimmed.fa"))


def test_missing_input_exits_255(tmp_path):
    r = run_cli([str(tmp_path / "nope.fastq")], tmp_path)
    assert r.returncode == 255 and r.stderr.decode().startswith("Error: file ")


def test_helpers_of_the_command_line(tmp_path):
    from mir_prefer_amd import trim
    assert [trim.parse_permille(x) for x in ("0", "0.1", ".25", "0.290", "0.999", "1", "0.1234", "", ".", "1.0")] == [0, 100, 250, 290, 999, None, None,
                                                                                                                    None, None, None]
    assert trim.output_name("d/lib.fastq.gz") == "d/lib.fastq.trimmed.fa" and trim.output_name("x.fa") == "x.fa.trimmed.fa"
    p = tmp_path / "m.fastq.gz"
    p.write_bytes(gzip.compress(b"@a\nAC") + gzip.compress(b"GT\n+\nIIII\n"))
    assert trim.read_input(str(p)) == b"@a\nACGT\n+\nIIII\n" and trim.first_byte(str(p)) == b"@"
    p.write_bytes(gzip.compress(b"@a\nACGT\n")[:-6] + b"xxxxxx")
    with pytest.raises(ValueError):
        trim.read_input(str(p))

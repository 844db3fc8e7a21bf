"""Host side of the tests of the trim kernel's two read paths and of its second adapter word (trim_kernels.hip; DESIGN.md §13, "Tests"): block_spans
restates which workgroups stage their reads in LDS and which read device memory; the generators build the inputs that tests/test_trim_paths_gpu.py
runs (reads long enough to leave the 32 KiB slab, four files around the slab limit, multi-line FASTA of long reads, adapters past 32 nt); the numpy
restatement is checked against the plain one on all of them, since it had only seen short reads; and the sensitivity conditions, computed from
adapter_pos alone, state what the inputs must contain for a wrong second adapter word to change an output."""
import functools
import os
import re

import numpy as np
import pytest

from tests.test_trim_cpu import ILLUMINA, ROOT, WS, adapter_pos, make_reads, parse, restate_trim, restate_trim_numpy, to_fasta, to_fastq
from tests.test_trim_gpu import OPTION_GRID, QUALITY_GRID

NT = 128          # TR_NT: reads per workgroup of trim_reads_kernel
SLAB = 32768      # TR_SLAB: bytes of a workgroup's LDS slab


# ---- the kernel's path rule

def _lines(data):
    """(start, end without the terminator) of every line, under split_lines' rule."""
    out, pos = [], 0
    for m in re.finditer(rb"\r\n|\r|\n", data):
        out.append((pos, m.start()))
        pos = m.end()
    if pos < len(data):
        out.append((pos, len(data)))
    return out


def _strip(data, b, e):
    while b < e and data[b] in WS:
        b += 1
    while e > b and data[e - 1] in WS:
        e -= 1
    return b, e


def block_spans(data, group=NT):
    """The span in bytes of every group of `group` consecutive reads as trim_reads_kernel computes it: from the smallest sequence start of the
    group, rounded down to 16, to the largest end.  FASTQ: offsets into the text, the end of a read is its stripped quality start + its length.
    FASTA: offsets into the gathered reads (the stripped lines of each record, concatenated), the end of a read is its own."""
    if not data:
        return []
    first, last = [], []
    if data[:1] == b"@":
        ln = _lines(data)
        while ln and _strip(data, *ln[-1])[0] == _strip(data, *ln[-1])[1]:
            ln.pop()
        for r in range(len(ln) // 4):
            sb, se = _strip(data, *ln[4 * r + 1])
            qb, _ = _strip(data, *ln[4 * r + 3])
            first.append(sb)
            last.append(qb + se - sb)
    else:
        off = 0
        for _, read, _ in parse(data)[1]:
            first.append(off)
            off += len(read)
            last.append(off)
    return [max(last[g:g + group]) - (min(first[g:g + group]) & ~15) for g in range(0, len(first), group)]


def predicted_paths(data):
    """(workgroups that stage their reads in LDS, workgroups that read device memory): what mirp_trim_last_paths reports."""
    spans = block_spans(data)
    return sum(s <= SLAB for s in spans), sum(s > SLAB for s in spans)


def test_block_spans_on_hand_written_files():
    data = b"@a twenty-byte header\nACGT\n+\nIIII\n@b\n  ACGTAC \n+\n IIIIII\n@c\nA\n+\nI\n"
    assert data[22:26] == b"ACGT" and data[39:45] == b"ACGTAC" and data[50:56] == b"IIIIII" and data[60:61] == b"A" and data[64:65] == b"I"
    # one group: the first sequence starts at 22 -> 16; the last quality starts at 64 and has 1 byte
    assert block_spans(data) == [65 - 16]
    # groups of two: {a, b} from 16 to b's stripped quality 50 + 6; {c} from 60 & ~15 = 48 to 65
    assert block_spans(data, 2) == [56 - 16, 65 - 48]
    # the trailing blank lines are no record; with \r\n the first sequence starts at 23 -> 16, and 11 line ends lie before the last quality
    assert block_spans(data + b"\n \n") == [49]
    assert block_spans(data.replace(b"\n", b"\r\n"), 3) == [65 + 11 - 16]
    # FASTA: reads of 20, 0 and 5 bases in the gathered buffer at 0, 20, 20
    fa = b">a b\nACGTACGTAC\n  GTACGTACGT \n>b\n\n>c x\r\nACG\r\nTT"
    assert [r for _, r, _ in parse(fa)[1]] == [b"ACGTACGTACGTACGTACGT", b"", b"ACGTT"]
    assert block_spans(fa) == [25] and block_spans(fa, 2) == [20, 25 - 16] and block_spans(fa, 1) == [20, 20 - 16, 25 - 16]
    assert block_spans(b"") == [] and predicted_paths(fa) == (1, 0)


def test_the_path_counter_is_declared_defined_and_bound():
    header = open(os.path.join(ROOT, "include", "mirprefer.h")).read()
    csrc = os.path.join(ROOT, "mir-prefer_amd", "csrc")
    assert "int mirp_trim_last_paths(const mirp_ctx* ctx, int64_t out[2]);" in header
    assert 'extern "C" int mirp_trim_last_paths(' in open(os.path.join(csrc, "mirp_trim.cpp")).read()
    assert "#define MIRP_ABI_VERSION 17 " in open(os.path.join(csrc, "mirp_api.cpp")).read()          # only entries are added
    kernels = open(os.path.join(csrc, "trim_kernels.hip")).read()
    assert "#define TR_NT %d " % NT in kernels and "#define TR_SLAB %d " % SLAB in kernels             # the constants block_spans restates
    from mir_prefer_amd import capi
    assert capi.ABI_VERSION == 17 and callable(capi.Context.trim_last_paths)


# ---- generators, shared with tests/test_trim_paths_gpu.py

def _bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.randint(0, len(alphabet), size=n)].tobytes()


def falling_quals(rng, n):
    """Phred+33 qualities that fall from about 41 to about 0 along the read, so that -q cuts into every read."""
    return bytes((np.clip(41 - (np.arange(n) * 42) // max(n, 1) + rng.randint(-6, 7, size=n), 0, 41) + 33).astype(np.uint8))


def fixed_reads(rng, names, length, adapter=ILLUMINA, err=0.05, alphabet=b"ACGTacgtN"):
    """Reads of exactly `length` bases planted as make_reads plants them: an insert, an adapter prefix (some with errors), and a random tail
    behind a whole adapter; length = one number or one per name."""
    ad = adapter.encode() if isinstance(adapter, str) else adapter
    out = []
    for i, name in enumerate(names):
        n = length if isinstance(length, int) else int(length[i])
        k = min(int(rng.randint(0, len(ad) + 1)), n)
        a = bytearray(ad[:k])
        for j in range(k):
            if rng.rand() < err:
                a[j] = b"ACGTN"[rng.randint(0, 5)]
        ins = int(rng.randint(0, n - k + 1)) if k == len(ad) else n - k
        seq = _bases(rng, ins, alphabet) + bytes(a) + _bases(rng, n - ins - k)
        out.append((name, seq, falling_quals(rng, n)))
    return out


def _renamed(prefix, reads):
    return [(prefix + n, s, q) for n, s, q in reads]


@functools.lru_cache(maxsize=None)
def paths_fastq():
    """805 reads whose groups of 128 are: 50 nt; 151 nt under 40-byte names; 101 nt under SRA-style headers; short reads around one 1,024-nt
    read; 251 nt; empty and 1-nt reads; 37 reads of 151 nt."""
    rng = np.random.RandomState(131)
    illumina = [(b"HWI-ST123:10:C0ABCACXX:1:1101:%d:%d" % (1000 + 7 * i, 2000 + i)).ljust(40, b"_") for i in range(128 + 37)]
    assert all(len(n) == 40 for n in illumina)
    sra = [b"SRR1234567.%d HWI-ST1234:100:C0ABCACXX:1:1101:%d:%d length=101" % (i + 1, 1000 + 7 * i, 2000 + i) for i in range(128)]
    short = _renamed(b"s", make_reads(rng, 127, hi=30, tail=(0, 10)))
    long_one = (b"long", _bases(rng, 1024 - len(ILLUMINA), b"ACGTacgtN") + ILLUMINA.encode(), falling_quals(rng, 1024))
    tiny = [(b"e%d" % i, b"", b"") if i % 2 == 0 else (b"o%d" % i, _bases(rng, 1), b"5") for i in range(128)]
    reads = (fixed_reads(rng, [b"a%d" % i for i in range(128)], 50) + fixed_reads(rng, illumina[:128], 151) + fixed_reads(rng, sra, 101) +
             short[:64] + [long_one] + short[64:] + fixed_reads(rng, [b"d%d extra" % i for i in range(128)], 251) + tiny + fixed_reads(rng, illumina[128:], 151))
    assert len(reads) == 128 * 6 + 37
    return to_fastq(reads)


PATHS_FASTQ_GROUPS = (False, True, True, False, True, False, False)       # the groups of paths_fastq that leave the slab

LIMIT_SPANS = (32752, 32768, 32769, 32784)
LIMIT_OPTIONS = [dict(adapter=ILLUMINA), dict(q=20, adapter=ILLUMINA, e_pm=250, overlap=1, min_len=0)]


@functools.lru_cache(maxsize=None)
def limit_file(span):
    """128 reads of 120 nt whose span is exactly `span` bytes (the second read's name is as long as that takes), then 40 short reads.  The first
    sequence starts at byte 9, so the span counts from byte 0: the kernel rounds the start down to 16."""
    def build(k):
        rng = np.random.RandomState(41)
        first = fixed_reads(rng, [b"lim%04d" % i for i in range(128)], 120)
        first[1] = (b"n" * k,) + first[1][1:]
        return to_fastq(first + _renamed(b"t", make_reads(rng, 40)))
    data = build(span - block_spans(build(0))[0])
    return data


@functools.lru_cache(maxsize=None)
def paths_fasta_reads():
    """Two groups of 128 reads of 300..1,024 nt, a group of short reads between them and 50 short reads behind."""
    rng = np.random.RandomState(132)
    out = []
    for g in range(2):
        lens = rng.randint(300, 421, size=128)
        lens[[5, 77, 100]] = (1024, 1023, 600) if g == 0 else (301, 1024, 777)
        out += fixed_reads(rng, [b"L%d_%d" % (g, i) + (b" words" if i % 4 == 0 else b"") for i in range(128)], lens)
        out += _renamed(b"s%d_" % g, make_reads(rng, 128 if g == 0 else 50))
    return out


FASTA_LAYOUTS = ((0, b"\n"), (60, b"\r\n"), (60, b"\n"), (0, b"\r\n"))


def paths_fasta(width, eol):
    return to_fasta(paths_fasta_reads(), eol, width)


@functools.lru_cache(maxsize=None)
def word_adapters():
    """Seeded ACGT adapters of 33, 48, 63 and 64 nt, and the 48-nt one in lower case."""
    rng = np.random.RandomState(1967)
    ads = [_bases(rng, m) for m in (33, 48, 63, 64)]
    return tuple(a.decode() for a in ads + [ads[1].lower()])


def word_options(adapter):
    m = len(adapter)
    return [dict(adapter=adapter, e_pm=100, overlap=3, min_len=0), dict(adapter=adapter, e_pm=0, overlap=33, min_len=0),
            dict(adapter=adapter, e_pm=250, overlap=m, min_len=0), dict(adapter=adapter, e_pm=16, overlap=33, min_len=0)]


@functools.lru_cache(maxsize=None)
def word_reads(adapter):
    """[(read, planted position)] for one adapter of m > 32 nt.
    grid      every insert length p in 0..130, 200, 511, 512, 513, 959, 960, 1024 - m x the adapter's prefix of length m, m - 1, min(m, 40), 33,
              with 0..3 substitutions from ACGTN, and a random tail behind a whole adapter; every fifth read in lower case
    targeted  for every offset k in 32..m - 1 the whole adapter with only offset k changed, to another base, to N and to n, at two insert
              lengths: one with p % 32 = 31, so that offset k is read from the third packed word, one elsewhere
    overlaps  for every l in 33..m a read that ends in the adapter's first l bases"""
    rng = np.random.RandomState(len(adapter) + (1000 if adapter.islower() else 0))
    ad = adapter.upper().encode()
    m = len(ad)
    out = []
    for pi, p in enumerate(list(range(131)) + [200, 511, 512, 513, 959, 960, 1024 - m]):
        for ki, k in enumerate((m, m - 1, min(m, 40), 33)):
            a = bytearray(ad[:k])
            for j in rng.choice(k, (pi + ki) % 4, replace=False):
                a[j] = b"ACGTN"[rng.randint(0, 5)]
            tail = _bases(rng, min(int(rng.randint(0, 31)), 1024 - p - k)) if k == m else b""
            seq = _bases(rng, p, b"ACGTacgtN") + bytes(a) + tail
            out.append((seq.lower() if len(out) % 5 == 4 else seq, p))
    for k in range(32, m):
        wrong = b"ACGT".replace(ad[k:k + 1], b"")[rng.randint(0, 3):][:1]
        for ch in (wrong, b"N", b"n"):
            for p in (31 + 32 * (k % 3), 64 * (k % 2) + (5 * k) % 32):
                out.append((_bases(rng, p) + ad[:k] + ch + ad[k + 1:] + _bases(rng, int(rng.randint(0, 11))), p))
    for ln in range(33, m + 1):
        p = 64 + (7 * ln) % 67
        out.append((_bases(rng, p) + ad[:ln], p))
    assert all(len(s) <= 1024 for s, _ in out)
    return tuple(out)


WORD_LAYOUTS = ("slab", "device")


@functools.lru_cache(maxsize=None)
def word_file(adapter, layout):
    """The reads of word_reads(adapter), shuffled, as FASTQ.  "slab": two short reads behind every one, so that every group of 128 fits the slab;
    "device": under 300-byte names, so that no whole group does."""
    rng = np.random.RandomState(7 + len(adapter))
    reads = [s for s, _ in word_reads(adapter)]
    rng.shuffle(reads)
    if layout == "device":
        return to_fastq([(b"w%d_" % i + b"x" * 300, s, b"I" * len(s)) for i, s in enumerate(reads)])
    fill = make_reads(rng, 2 * len(reads), adapter=adapter.upper()[:20], lo=0, hi=12, tail=(0, 5))
    recs = []
    for i, s in enumerate(reads):
        recs += [(b"w%d" % i, s, b"I" * len(s)), fill[2 * i], fill[2 * i + 1]]
    return to_fastq(recs)


# ---- the reference, computed once per (input, options) and shared by both files

@functools.lru_cache(maxsize=None)
def _reference(data, kw):
    return restate_trim(data, **dict(kw))


def reference(data, **kw):
    """restate_trim(data, **kw) -> (output bytes, stats); cached, not to be modified."""
    return _reference(data, tuple(sorted(kw.items())))


# ---- the inputs are what the GPU tests need them to be

def test_path_files_have_groups_on_both_sides_of_the_slab():
    spans = block_spans(paths_fastq())
    assert tuple(s > SLAB for s in spans) == PATHS_FASTQ_GROUPS and predicted_paths(paths_fastq()) == (4, 3)
    n_reads = len(parse(paths_fastq())[1])
    assert n_reads % NT == 37 and len(spans) == n_reads // NT + 1
    assert 2048 < spans[3] <= SLAB                                      # the 1,024-nt read among short reads stays in the slab
    for width, eol in FASTA_LAYOUTS:
        data = paths_fasta(width, eol)
        over = [s > SLAB for s in block_spans(data)]
        assert over == [True, False, True, False] and len(parse(data)[1]) % NT == 50
        assert parse(data) == parse(paths_fasta(0, b"\n"))            # the same names and reads in every layout, so one reference serves all four
    lens = [len(r) for _, r, _ in paths_fasta_reads() if len(r) >= 300]
    assert len(lens) == 256 and min(lens) == 300 and max(lens) == 1024
    assert max(len(ln) for ln in paths_fasta(60, b"\n").split(b"\n") if ln[:1] != b">") == 60


def test_limit_files_sit_on_the_slab_limit():
    for span in LIMIT_SPANS:
        data = limit_file(span)
        spans = block_spans(data)
        assert spans == [span, spans[1]] and spans[1] < SLAB
        # told without block_spans: the first sequence starts at byte 9 (rounded down: 0), and the last quality of the group ends one byte
        # before the header of read 129
        assert data.index(b"\n") + 1 == 9 and data.index(b"@tr0") - 1 == span
        assert predicted_paths(data) == ((2, 0) if span <= SLAB else (1, 1))
    assert len({limit_file(s).replace(b"n", b"") for s in LIMIT_SPANS}) == 1     # the four differ in the length of that one name only


def test_word_files_are_on_the_path_they_are_named_after():
    for ad in word_adapters():
        n = len(word_reads(ad))
        slab, dev = predicted_paths(word_file(ad, "slab"))
        assert dev == 0 and slab == (3 * n + NT - 1) // NT
        slab, dev = predicted_paths(word_file(ad, "device"))
        assert dev >= n // NT >= 4 and slab <= 1
        planted = {s for s, _ in word_reads(ad)}
        for layout in WORD_LAYOUTS:
            assert sorted(r for _, r, _ in parse(word_file(ad, layout))[1] if r in planted) == sorted(s for s, _ in word_reads(ad))


def test_word_adapters_use_the_second_word():
    ads = word_adapters()
    assert [len(a) for a in ads] == [33, 48, 63, 64, 48] and ads[4] == ads[1].lower() != ads[1]
    for a in ads:
        assert set(a.upper()) <= set("ACGT") and set(a[32:].upper()) != {"A"}
        assert "G" in a[32:].upper()          # N and n carry G's 2-bit code: only under a G does a lost non-ACGT mask turn them into a match


# ---- yardstick: the numpy restatement had only seen short reads

@pytest.mark.parametrize("which", ["paths", "limits"] + ["words%d" % i for i in range(5)])
def test_numpy_restatement_agrees_on_the_new_inputs(which):
    if which == "paths":
        cases = [(paths_fastq(), kw) for kw in OPTION_GRID + QUALITY_GRID]
    elif which == "limits":
        cases = [(limit_file(s), kw) for s in LIMIT_SPANS for kw in LIMIT_OPTIONS]
    else:
        ad = word_adapters()[int(which[5:])]
        cases = [(word_file(ad, layout), kw) for layout in WORD_LAYOUTS for kw in word_options(ad)]
    for data, kw in cases:
        assert restate_trim_numpy(data, **kw) == reference(data, **kw), kw


# ---- sensitivity: what the word inputs must contain, from adapter_pos alone

@functools.lru_cache(maxsize=None)
def _found(adapter):
    """[[adapter_pos under each of word_options(adapter)] per read of word_reads(adapter)]."""
    return [[adapter_pos(s, kw["adapter"].encode(), kw["e_pm"], kw["overlap"]) for kw in word_options(adapter)] for s, _ in word_reads(adapter)]


def _replace_n(seq, p, ad, base=None):
    """seq with every N / n at adapter offsets >= 32 of the adapter planted at p replaced by the adapter's own base (or by `base`)."""
    b = bytearray(seq)
    for i in range(p + 32, min(p + len(ad), len(b))):
        if b[i] in b"Nn":
            b[i] = base if base is not None else ad[i - p]
    return bytes(b)


@pytest.mark.parametrize("i", range(5))
def test_word_reads_are_sensitive_to_the_second_word(i):
    adapter = word_adapters()[i]
    ad = adapter.upper().encode()
    m = len(ad)
    reads, found, opts = word_reads(adapter), _found(adapter), word_options(adapter)
    every = [(len(s), p) for (s, _), row in zip(reads, found) for p in row if p is not None]
    overlaps = {min(m, n - p) for n, p in every}
    assert set(range(33, m + 1)) <= overlaps                           # every overlap that reaches into the second word is matched somewhere
    assert {p % 32 for _, p in every if p >= 64} == set(range(32))    # every alignment of the window to the packed words, past the first refill
    assert all(any(p >= lim for _, p in every) for lim in (96, 512, 960))
    if m < 48:
        return
    # the first word alone gives another answer
    first_word = sum(any(adapter_pos(s, ad[:32], kw["e_pm"], min(kw["overlap"], 32)) != f for kw, f in zip(opts, row)) for (s, _), row in zip(reads, found))
    assert first_word >= 200, first_word
    # a non-ACGT byte under the second word decides: replaced by the adapter's base, and by G (whose 2-bit code N and n carry)
    for base in (None, ord("G")):
        changed = sum(any(adapter_pos(_replace_n(s, p, ad, base), ad, kw["e_pm"], kw["overlap"]) != f for kw, f in zip(opts, row))
                      for (s, p), row in zip(reads, found) if _replace_n(s, p, ad, base) != s)
        assert changed >= 10, (base, changed)


def test_all_overlaps_33_to_64_are_matched():
    seen = set()
    for adapter in word_adapters():
        m = len(adapter)
        seen |= {min(m, len(s) - p) for (s, _), row in zip(word_reads(adapter), _found(adapter)) for p in row if p is not None}
    assert set(range(33, 65)) <= seen


def test_floor_at_e16_decides_between_62_and_63():
    """16 * 62 // 1000 = 0 and 16 * 63 // 1000 = 1: one error is allowed in an overlap of 63 but not of 62; both reach into the second word."""
    assert 16 * 62 // 1000 == 0 and 16 * 63 // 1000 == 1
    ad = word_adapters()[3].encode()
    hit = ad[:40] + b"N" + ad[41:63]
    assert adapter_pos(b"ACGT" + hit, ad, 16, 33) == 4 and adapter_pos(b"ACGT" + hit[:62], ad, 16, 33) is None
    for adapter in word_adapters()[2:4]:
        rows = [(len(s) - p, row[3], row[1]) for (s, p), row in zip(word_reads(adapter), _found(adapter)) if len(s) - p == 63]
        assert any(e16 is not None and e0 is None for _, e16, e0 in rows), adapter      # found only thanks to the one allowed error

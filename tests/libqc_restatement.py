"""Restatements of the library profile (`python -m mir_prefer_amd.libqc`, mirp_libqc_reads), which define its output: a plain-Python
one that follows the definition rule by rule, and a numpy one (np.bincount on rolling codes) for the larger inputs.  Both take the parsed reads of
tests/test_trim_cpu.parse, so the input rules and refusals are the trim's.  restate_libqc / restate_libqc_numpy -> the dict that
capi.Context.libqc_reads returns, without `seconds` and with the k-mer table; render() -> the three files of the verb."""
import numpy as np

from tests.test_trim_cpu import adapter_pos, parse, restate_trim_numpy

K, W = 12, 64
CODES = 4 ** K
LIMIT = 1024
MIN_COUNT = 16
LEFT_CAP, RIGHT_CAP = 1024, 1024 + 64
ADAPTER_MAX = 64
SAMPLE = 1 << 20
NONE, OK, UNSURE = "none", "ok", "unsure"
STOPS = ("purity", "support", "cap")
ACGT = "ACGT"


def code_of(kmer):
    c = 0
    for ch in kmer:
        c = c * 4 + ACGT.index(ch)
    return c


def kmer_of(code):
    return "".join(ACGT[(code >> (2 * (K - 1 - i))) & 3] for i in range(K))


# ---- the k-mer table

def table_plain(reads, sample=SAMPLE):
    """reads = [bytes]; -> the 4^12 counters (uint32)."""
    counts = {}
    for read in reads[:sample]:
        s = read[:W].upper().decode("ascii")
        for p in range(len(s) - K + 1):
            kmer = s[p:p + K]
            counts[kmer] = counts.get(kmer, 0) + 1
    table = np.zeros(CODES, np.uint32)
    for kmer, c in counts.items():
        if all(ch in ACGT for ch in kmer):
            table[code_of(kmer)] = c
    return table


_CLASS = np.full(256, 4, np.int64)
for _i, _ch in enumerate(b"ACGT"):
    _CLASS[_ch] = _i
    _CLASS[_ch + 32] = _i


def _matrix(reads, width):
    """(classes [n, width] with 5 behind the read's end, lengths)."""
    n = len(reads)
    lens = np.array([len(r) for r in reads], np.int64).reshape(n)
    m = np.full((n, width), 5, np.int64)
    if n and width:
        flat = np.frombuffer(b"".join(r[:width] for r in reads), np.uint8)
        ln = np.minimum(lens, width)
        rows = np.repeat(np.arange(n), ln)
        cols = np.arange(len(flat)) - np.repeat(np.cumsum(ln) - ln, ln)
        m[rows, cols] = _CLASS[flat]
    return m, lens


def table_numpy(reads, sample=SAMPLE):
    reads = reads[:sample]
    cls, _ = _matrix(reads, W)
    codes = [np.zeros(0, np.int64)]
    if len(reads):
        good = cls < 4
        code = np.zeros(len(reads), np.int64)
        run = np.zeros(len(reads), np.int64)
        for j in range(W):
            code = ((code << 2) | (cls[:, j] & 3)) & (CODES - 1)
            run = np.where(good[:, j], run + 1, 0)
            codes.append(code[run >= K])
    table = np.bincount(np.concatenate(codes), minlength=CODES)
    assert table.max(initial=0) < 2 ** 32
    return table.astype(np.uint32)


# ---- the adapter, from the table alone

def eligible(kmer):
    return max(kmer.count(b) for b in ACGT) <= 6


_ELIGIBLE = None


def eligible_mask():
    global _ELIGIBLE
    if _ELIGIBLE is None:
        codes = np.arange(CODES, dtype=np.int64)
        counts = np.zeros((4, CODES), np.int8)
        for i in range(K):
            b = (codes >> (2 * i)) & 3
            for x in range(4):
                counts[x] += b == x
        _ELIGIBLE = counts.max(axis=0) <= 6
    return _ELIGIBLE


def find_adapter(table, n_reads):
    """The walk on the counters -> dict(adapter, status, seed, seed_count, min_count, left_steps, left_stop)."""
    masked = np.where(eligible_mask(), table.astype(np.int64), -1)
    seed_code = int(np.argmax(masked))                      # the first of the largest: ties to the smallest code
    c_seed = int(masked[seed_code])
    seed = kmer_of(seed_code)
    assert eligible(seed)
    none = dict(adapter="", status=NONE, seed=seed, seed_count=c_seed, min_count=0, left_steps=0, left_stop=STOPS[0])
    if c_seed < MIN_COUNT or n_reads == 0:
        return none
    minc = max(MIN_COUNT, c_seed // 64)

    def step(make):
        cs = [int(table[code_of(make(b))]) for b in ACGT]
        m, t = max(cs), sum(cs)
        if m < minc:
            return None, "support"
        if 5 * m < 4 * t:
            return None, "purity"
        return ACGT[cs.index(m)], None                      # ties to the first of A, C, G, T

    s, left_stop = seed, "cap"
    while len(s) < LEFT_CAP:
        b, why = step(lambda b: b + s[:K - 1])
        if b is None:
            left_stop = why
            break
        s = b + s
    left_steps = len(s) - K
    while len(s) < RIGHT_CAP:
        b, why = step(lambda b: s[-(K - 1):] + b)
        if b is None:
            break
        s = s + b
    return dict(adapter=s[:ADAPTER_MAX], status=OK if left_stop == "purity" else UNSURE, seed=seed, seed_count=c_seed, min_count=minc,
                left_steps=left_steps, left_stop=left_stop)


# ---- the tables

def _used_adapter(found, adapter):
    adapter = adapter.decode() if isinstance(adapter, bytes) else adapter
    return adapter if adapter else found["adapter"]


def _overlap(overlap, m):
    return min(3 if overlap is None else overlap, m)


def _empty():
    return np.zeros(LIMIT + 1, np.int64), np.zeros((LIMIT, 6), np.int64), np.zeros((LIMIT + 1, 6), np.int64)


def restate_libqc(data, adapter="", e_pm=100, overlap=None, sample=SAMPLE):
    """Plain Python; Refused as tests/test_trim_cpu.parse raises it."""
    fq, recs = parse(data)
    reads = [r for _, r, _ in recs]
    table = table_plain(reads, sample)
    found = find_adapter(table, len(reads))
    used = _used_adapter(found, adapter)
    raw_len, cycles, insert = _empty()
    with_adapter = dimers = 0
    for _, read, qual in recs:
        raw_len[len(read)] += 1
        up = read.upper()
        for i, ch in enumerate(up):
            cycles[i][b"ACGT".index(ch) if ch in b"ACGT" else 4] += 1
            if fq:
                cycles[i][5] += qual[i] - 33
        if used:
            p = adapter_pos(read, used.encode(), e_pm, _overlap(overlap, len(used)))
            if p is not None:
                with_adapter += 1
                dimers += p == 0
            else:
                p = len(read)
            insert[p][4 if p == 0 or up[0] not in b"ACGT" else b"ACGT".index(up[0])] += 1
            insert[p][5] += 1
    return dict(found, reads=len(reads), sampled=min(len(reads), sample), with_adapter=with_adapter, dimers=dimers, raw_len=raw_len, cycles=cycles,
                insert=insert, table=table)


def restate_libqc_numpy(data, adapter="", e_pm=100, overlap=None, sample=SAMPLE):
    fq, recs = parse(data)
    reads = [r for _, r, _ in recs]
    n = len(reads)
    table = table_numpy(reads, sample)
    found = find_adapter(table, n)
    used = _used_adapter(found, adapter)
    raw_len, cycles, insert = _empty()
    width = max([len(r) for r in reads] + [1])
    cls, lens = _matrix(reads, width)
    raw_len += np.bincount(lens, minlength=LIMIT + 1)
    for x in range(5):
        cycles[:width, x] = (cls == x).sum(axis=0)
    if fq and n:
        flat = np.frombuffer(b"".join(ql for _, _, ql in recs), np.uint8).astype(np.int64) - 33
        cols = np.arange(len(flat)) - np.repeat(np.cumsum(lens) - lens, lens)
        cycles[:, 5] = np.bincount(cols, weights=flat, minlength=LIMIT).astype(np.int64)
    with_adapter = dimers = 0
    if used and n:
        # the cut of every read: the lengths of the records the trim's numpy restatement writes with no filter.  It takes FASTQ alone, so the reads
        # go in as FASTQ of their own, behind them a read of one N, which no adapter matches: an empty last read would be a blank tail
        fastq = b"".join(b"@x\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in reads + [b"N"])
        out, st = restate_trim_numpy(fastq, adapter=used.encode(), e_pm=e_pm, overlap=_overlap(overlap, len(used)), min_len=0)
        cut = np.array([len(ln) for ln in out.split(b"\n")[1::2]], np.int64)
        assert len(cut) == n + 1 and st["written"] == n + 1 and cut[n] == 1
        cut = cut[:n]
        first = np.where(cut == 0, 4, np.minimum(cls[:, 0], 4))
        np.add.at(insert, (cut, first), 1)
        insert[:, 5] = np.bincount(cut, minlength=LIMIT + 1)
        with_adapter = st["adapter"]
        dimers = int(((cut == 0) & (lens > 0)).sum())
    return dict(found, reads=n, sampled=min(n, sample), with_adapter=with_adapter, dimers=dimers, raw_len=raw_len, cycles=cycles, insert=insert,
                table=table)


def same(a, b):
    """Whether two results are equal in every entry."""
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


# ---- the verb's files

def insert_mode(insert):
    """The insert length with the most reads among the lengths past 0, ties to the shortest; 0 when there is none."""
    tot = insert[1:, 5]
    return int(np.argmax(tot)) + 1 if tot.max(initial=0) > 0 else 0


def render(res):
    """(X.libqc.tsv, X.libqc.lengths.tsv, X.libqc.cycles.tsv) as bytes."""
    keys = [("reads", res["reads"]), ("sampled", res["sampled"]), ("adapter", res["adapter"]), ("status", res["status"]), ("seed", res["seed"]),
            ("seed_count", res["seed_count"]), ("left_steps", res["left_steps"]), ("left_stop", res["left_stop"]), ("with_adapter", res["with_adapter"]),
            ("dimers", res["dimers"]), ("insert_mode", insert_mode(res["insert"]))]
    summary = "".join("%s\t%s\n" % kv for kv in keys)
    raw, ins, cyc = res["raw_len"], res["insert"], res["cycles"]
    top = max([i for i in range(LIMIT + 1) if raw[i] or ins[i][5]], default=0)
    lengths = "length\traw\tinserts\tA\tC\tG\tT\tother\n" + "".join(
        "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (i, raw[i], ins[i][5], ins[i][0], ins[i][1], ins[i][2], ins[i][3], ins[i][4]) for i in range(top + 1))
    rows = []
    for i in range(LIMIT):
        n = int(sum(cyc[i][:5]))
        if n == 0:
            break
        milli = (2000 * int(cyc[i][5]) + n) // (2 * n)                 # the mean to three decimals, half up, in integers
        rows.append("%d\t%d\t%d\t%d\t%d\t%d\t%d.%03d\n" % ((i + 1,) + tuple(int(x) for x in cyc[i][:5]) + (milli // 1000, milli % 1000)))
    cycles = "cycle\tA\tC\tG\tT\tother\tmean_quality\n" + "".join(rows)
    return summary.encode(), lengths.encode(), cycles.encode()

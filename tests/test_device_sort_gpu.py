"""GPU tests of the stable device sort (mir-prefer_amd/csrc/sort_kernels.hip) on its own, through the hooks mirp_sort_u64, mirp_sort_records and
mirp_sort_alns: the three instantiations of device_radix_sort that the ingest, the read collapse, the align index and every key pass run through.

The reference is numpy: order = np.argsort(digit_key, kind="stable"), where digit_key is the key restricted to the bits the sort is specified to
order by -- whole 8-bit digits, the key bits [base, base + 8 * ceil(bits / 8)) -- computed in uint64.  The whole output must equal input[order],
payload included: every record carries its input index outside the sorted bits (as far as there is room), so a rank that is right as a set but
wrong in order shows, and the other bits outside the sorted range are random and must not matter.  Widths that are no multiple of 8 get random
bits above `bits` and are expected in the order of the rounded-up width: that is the contract the callers in clusters_kernels.hip rely on.

Sizes sit on the edges the kernels have: 64 records per ballot step, 2,048 per wave tile, 8,192 per workgroup (with idle waves in the last one),
64 against 65 tiles (256 * tiles counters pass 16,384 and the scan changes kernels), and one size near 10^6 that is no multiple of 64."""
import ctypes as C

import numpy as np
import pytest

from mir_prefer_amd.capi import SORT_REC_DTYPE, MirpError
from mir_prefer_amd.synth import ALN_DTYPE

pytestmark = pytest.mark.gpu

U64 = np.uint64
SIZES = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 2048 + 1, 64 * 2048, 64 * 2048 + 1, 1_000_003)
EDGES = (0, 1, 64, 65, 2048, 2049, 8192, 8193, 3 * 8192 + 2048 + 1, 64 * 2048, 64 * 2048 + 1, 1_000_003)      # one of every edge class, for the wider records
PATTERN_SIZES = (65, 2049, 8193, 3 * 8192 + 2048 + 1, 64 * 2048 + 1)
INDEX_BITS = 20                                                                                              # every size is below 2^20


def rounded(bits):
    return (bits + 7) // 8 * 8


def mask(bits):
    return U64((1 << bits) - 1) if bits < 64 else U64(0xffffffffffffffff)


def rand64(rng, n):
    return (rng.integers(0, 1 << 32, n, dtype=U64) << U64(32)) | rng.integers(0, 1 << 32, n, dtype=U64)


# ---------------------------------------------------------------------------------------------------- key patterns over a field of `bits` bits
def p_uniform(rng, n, bits):
    return rand64(rng, n) & mask(bits)


def p_equal(rng, n, bits):
    return np.full(n, rand64(rng, 1)[0] & mask(bits), dtype=U64)


def p_alternating(rng, n, bits):
    v = rand64(rng, 2) & mask(bits)
    return v[np.arange(n) & 1]


def p_runs(rng, n, bits):
    """3 to 5 distinct values in long runs: heavy duplicates, and runs that cross tile edges"""
    v = rand64(rng, int(rng.integers(3, 6))) & mask(bits)
    return v[(np.arange(n) // max(1, n // 11)) % len(v)]


def p_sorted(rng, n, bits):
    return np.sort(p_uniform(rng, n, bits))


def p_reverse(rng, n, bits):
    return p_sorted(rng, n, bits)[::-1].copy()


def p_top_digit(rng, n, bits):
    top = 8 * ((bits - 1) // 8)
    return ((rand64(rng, 1)[0] & mask(top)) | (rng.integers(0, 256, n, dtype=U64) << U64(top))) & mask(bits)


def p_bottom_digit(rng, n, bits):
    return ((rand64(rng, 1)[0] & ~U64(255)) | rng.integers(0, 256, n, dtype=U64)) & mask(bits)


def p_extremes(rng, n, bits):
    """every digit is 0, 255 or random, a third each: digit values 0 and 255 are present in every pass"""
    out = np.zeros(n, dtype=U64)
    for d in range(rounded(bits) // 8):
        pick = rng.integers(0, 3, n)
        digit = np.where(pick == 0, 0, np.where(pick == 1, 255, rng.integers(0, 256, n))).astype(U64)
        out |= digit << U64(8 * d)
    return out


PATTERNS = (p_equal, p_alternating, p_runs, p_sorted, p_reverse, p_top_digit, p_bottom_digit, p_extremes)


def field(rng, pattern, n, bits):
    """a pattern over `bits` bits; where `bits` is no multiple of 8, random bits above it up to the whole digit (p_extremes fills the whole digits itself)"""
    w = rounded(bits)
    f = pattern(rng, n, w if pattern is p_extremes else bits)
    if w > bits and pattern is not p_extremes:
        f |= (rand64(rng, n) & mask(w - bits)) << U64(bits)
    if pattern is p_extremes and n >= 2048:
        for d in range(w // 8):
            digits = (f >> U64(8 * d)) & U64(255)
            assert (digits == 0).any() and (digits == 255).any()
    return f


def payload(rng, n):
    """the input index in the low INDEX_BITS bits, random bits above"""
    return np.arange(n, dtype=U64) | (rand64(rng, n) << U64(INDEX_BITS))


def cases(sizes):
    """(pattern, n): the uniform keys at every size, every other pattern at three of the pattern sizes, the scan-kernel switch among them"""
    for n in sizes:
        yield p_uniform, n
    for k, pattern in enumerate(PATTERNS):
        for n in PATTERN_SIZES[k % 2:4:2] + PATTERN_SIZES[-1:]:
            yield pattern, n


# ---------------------------------------------------------------------------------------------------- u64
def make_u64(rng, pattern, n, base, bits):
    """keys in the bits [base, base + w), w = the rounded width; the payload fills the bits below base and, where there are any, above base + w"""
    w = min(rounded(bits), 64 - base)
    v = (field(rng, pattern, n, bits) & mask(w)) << U64(base)
    p = payload(rng, n)
    v |= p & mask(base)
    if base + w < 64:
        v |= (p >> U64(base)) << U64(base + w)
    return v


def digit_key_u64(v, base, bits):
    if bits == 0:
        return np.zeros(len(v), dtype=U64)
    return (v >> U64(base)) & mask(rounded(bits))


@pytest.mark.parametrize("base,bits", [(0, 8), (0, 24), (0, 64), (32, 32), (4, 56), (0, 21)])
def test_u64_sizes_patterns_and_widths(gpu_ctx, base, bits):
    rng = np.random.default_rng(1000 * base + bits)
    for pattern, n in cases(SIZES):
        v = make_u64(rng, pattern, n, base, bits)
        want = v[np.argsort(digit_key_u64(v, base, bits), kind="stable")]
        got = gpu_ctx.sort_u64(v, base, bits)
        assert got.dtype == U64 and np.array_equal(got, want), (pattern.__name__, n, base, bits, int(np.flatnonzero(got != want)[0]))


def test_u64_payload_shows_the_order_within_equal_keys(gpu_ctx):
    """what the tests above rely on, said once by hand: with the index below base, equal keys come out with rising indices, at every edge size"""
    for n in SIZES:
        v = (U64(3) << U64(32)) | np.arange(n, dtype=U64)
        v[1::2] |= U64(1) << U64(40)
        got = gpu_ctx.sort_u64(v, 40, 8)                             # one pass: two reversals of a tie would cancel
        half = (n + 1) // 2
        assert np.array_equal(got[:half] & mask(32), np.arange(0, n, 2, dtype=U64)) and np.array_equal(got[half:] & mask(32), np.arange(1, n, 2, dtype=U64)), n


# ---------------------------------------------------------------------------------------------------- 16-byte records
def make_records(rng, pattern, n, bits):
    w = rounded(bits)
    r = np.zeros(n, dtype=SORT_REC_DTYPE)
    r["key"] = field(rng, pattern, n, bits)
    if w < 64:
        r["key"] |= rand64(rng, n) << U64(w)                       # outside the sorted bits
    r["a"] = np.arange(n, dtype=np.uint32)
    r["b"] = ~np.arange(n, dtype=np.uint32)
    return r


@pytest.mark.parametrize("bits", [64, 33, 21])
def test_records_sizes_patterns_and_widths(gpu_ctx, bits):
    rng = np.random.default_rng(7000 + bits)
    for pattern, n in cases(EDGES):
        r = make_records(rng, pattern, n, bits)
        want = r[np.argsort(r["key"] & mask(rounded(bits)), kind="stable")]
        got = gpu_ctx.sort_records(r, bits)
        assert got.dtype == SORT_REC_DTYPE and got.tobytes() == want.tobytes(), (pattern.__name__, n, bits)


# ---------------------------------------------------------------------------------------------------- MirpAln
def make_alns(rng, pattern, n, posbits, tidbits):
    f = field(rng, pattern, n, posbits + tidbits)
    idx = np.arange(n, dtype=np.uint32)
    a = np.zeros(n, dtype=ALN_DTYPE)
    a["pos"] = (f & mask(posbits)).astype(np.int64).astype(np.int32)
    a["tid"] = (f >> U64(posbits)).astype(np.int64).astype(np.int32)
    a["depth"] = idx ^ np.uint32(0xa5a5a5a5)                        # the index, spread over the four fields that are not sorted by
    a["len"] = (idx & 0xffff).astype(np.uint16)
    a["strand"] = ((idx >> 16) & 0xff).astype(np.uint8)
    a["sample"] = ((idx >> 3) & 0xff).astype(np.uint8)
    return a


def digit_key_alns(a, posbits, tidbits):
    key = (a["tid"].astype(np.uint32).astype(U64) << U64(posbits)) | a["pos"].astype(np.uint32).astype(U64)
    return key & mask(rounded(posbits + tidbits))


@pytest.mark.parametrize("posbits,tidbits", [(8, 0), (20, 4), (31, 17)])
def test_alns_sizes_patterns_and_widths(gpu_ctx, posbits, tidbits):
    rng = np.random.default_rng(9000 + 100 * posbits + tidbits)
    for pattern, n in cases(EDGES):
        a = make_alns(rng, pattern, n, posbits, tidbits)
        assert n == 0 or (0 <= a["pos"].min() and int(a["pos"].max()) < 1 << posbits and 0 <= a["tid"].min() and int(a["tid"].max()) < 1 << tidbits)
        want = a[np.argsort(digit_key_alns(a, posbits, tidbits), kind="stable")]
        got = gpu_ctx.sort_alns(a, posbits, tidbits)
        assert got.dtype == ALN_DTYPE and got.tobytes() == want.tobytes(), (pattern.__name__, n, posbits, tidbits)


# ---------------------------------------------------------------------------------------------------- reuse of the context's scratch
def test_60_calls_back_to_back_on_one_context(gpu_ctx):
    """The counters (sort_counts) and the ticket state of the look-back scan belong to the context and are reused from call to call: sizes that
    alternate across the scan-kernel switch (35 and 1 tiles against 98 and 489) and across the growth of the counters, all three record types."""
    rng = np.random.default_rng(60)
    sizes = (70_001, 200_003, 513, 1_000_003)
    inputs = []
    for n in sizes:
        v = make_u64(rng, p_uniform if n != 513 else p_runs, n, 0, 24)
        inputs.append(("u64", v, v[np.argsort(digit_key_u64(v, 0, 24), kind="stable")]))
    r = make_records(rng, p_runs, 200_003, 21)
    inputs.append(("rec", r, r[np.argsort(r["key"] & mask(24), kind="stable")]))
    a = make_alns(rng, p_uniform, 70_001, 20, 4)
    inputs.append(("aln", a, a[np.argsort(digit_key_alns(a, 20, 4), kind="stable")]))
    for call in range(60):
        kind, v, want = inputs[call % len(inputs)]
        got = gpu_ctx.sort_u64(v, 0, 24) if kind == "u64" else gpu_ctx.sort_records(v, 21) if kind == "rec" else gpu_ctx.sort_alns(v, 20, 4)
        assert got.tobytes() == want.tobytes(), (call, kind, len(v))


# ---------------------------------------------------------------------------------------------------- the edges of the arguments
def test_nothing_to_sort_leaves_the_input(gpu_ctx):
    rng = np.random.default_rng(5)
    v = rand64(rng, 5000)
    assert np.array_equal(gpu_ctx.sort_u64(v, 0, 0), v) and np.array_equal(gpu_ctx.sort_u64(v, 64, 0), v) and np.array_equal(gpu_ctx.sort_u64(v, 17, 0), v)
    r = make_records(rng, p_uniform, 5000, 64)
    assert gpu_ctx.sort_records(r, 0).tobytes() == r.tobytes()
    a = make_alns(rng, p_uniform, 5000, 20, 4)
    assert gpu_ctx.sort_alns(a, 0, 0).tobytes() == a.tobytes()
    assert len(gpu_ctx.sort_u64(v[:0], 0, 64)) == 0 and len(gpu_ctx.sort_records(r[:0], 64)) == 0 and len(gpu_ctx.sort_alns(a[:0], 31, 17)) == 0


def _raw(ctx, name, src, n, widths, dst):
    fn = getattr(ctx.lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int32] * len(widths) + [C.c_void_p]
    rc = fn(ctx.h, src, n, *widths, dst)
    return rc, ctx.lib.mirp_last_error(ctx.h).decode()


def test_refusals_leave_the_context_usable(gpu_ctx):
    buf = np.arange(64, dtype=U64)[::-1].copy()
    out = np.full(128, 77, dtype=U64)                                # 64 records of the widest type
    p, q = buf.ctypes.data, out.ctypes.data
    bad = [("mirp_sort_u64", p, -1, (0, 8), q), ("mirp_sort_u64", None, 8, (0, 8), q), ("mirp_sort_u64", p, 8, (0, 8), None),
           ("mirp_sort_u64", p, 8, (-1, 8), q), ("mirp_sort_u64", p, 8, (0, -1), q), ("mirp_sort_u64", p, 8, (33, 32), q),
           ("mirp_sort_u64", p, 8, (64, 1), q), ("mirp_sort_u64", p, 8, (0, 65), q), ("mirp_sort_u64", p, 8, (2 ** 31 - 1, 2 ** 31 - 1), q),
           ("mirp_sort_records", p, -1, (8,), q), ("mirp_sort_records", None, 4, (8,), q), ("mirp_sort_records", p, 4, (8,), None),
           ("mirp_sort_records", p, 4, (-1,), q), ("mirp_sort_records", p, 4, (65,), q),
           ("mirp_sort_alns", p, -1, (8, 8), q), ("mirp_sort_alns", None, 4, (8, 8), q), ("mirp_sort_alns", p, 4, (8, 8), None),
           ("mirp_sort_alns", p, 4, (-1, 8), q), ("mirp_sort_alns", p, 4, (8, -1), q), ("mirp_sort_alns", p, 4, (40, 30), q),
           ("mirp_sort_alns", p, 4, (33, 0), q), ("mirp_sort_alns", p, 4, (0, 33), q)]
    for name, src, n, widths, dst in bad:
        rc, msg = _raw(gpu_ctx, name, src, n, widths, dst)
        assert rc == -1 and msg.startswith(name + ":"), (name, n, widths, rc, msg)
        assert (out == 77).all()
        assert np.array_equal(gpu_ctx.sort_u64(buf, 0, 8), buf[::-1])                       # the context goes on sorting
    rc, _ = _raw(gpu_ctx, "mirp_sort_u64", None, 0, (0, 64), None)                           # nothing, from nowhere: fine
    assert rc == 0
    with pytest.raises(MirpError, match=r"mirp_sort_u64 failed \(-1\)"):
        gpu_ctx.sort_u64(buf, 60, 8)

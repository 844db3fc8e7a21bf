"""GPU parity of the tail-free chunked fold (set_fold_overlap_tailfree: the fills of neighbouring chunks on two streams, a candidate-pool pass per chunk
only, the dense hand-offs folded chunk by chunk behind the last epilogue; per-chunk counter blocks and dense lists).  Every case folds the same
sequences three ways -- tail-free with a small chunk override, the ordered schedule (mode 0) with the same override, the serial path
(set_fold_overlap(0)) -- and the three agree exactly: line count, every line (text, energy, start column, printed flag), MFE and status of every
window, last_fold_dense() and last_fold_fallbacks().  One case per family is also checked against the CPU oracle."""
import random
import time

import numpy as np
import pytest

from tests import seqgen
from tests.test_fold_overlap_gpu import GC, TANDEM, _oracle, _same

pytestmark = pytest.mark.gpu


def _fold(ctx, seqs, span, overlap, tailfree, max_lines=96):
    """(raw arrays, chunks, windows handed to the dense kernel, windows handed to the generic kernel) with the two switches set"""
    try:
        ctx.set_fold_overlap(overlap)
        ctx.set_fold_overlap_tailfree(tailfree)
        raw = ctx.fold_batch_raw(seqs, span, max_lines)
        return raw, ctx.last_fold_overlap_chunks(), ctx.last_fold_dense(), ctx.last_fold_fallbacks()
    finally:
        ctx.set_fold_overlap(-1)
        ctx.set_fold_overlap_tailfree(-1)


def _three(ctx, seqs, span, chunk, chunks):
    """tail-free == ordered == serial; -> (the tail-free arrays, dense, generic)"""
    a, chunks_a, dense_a, gen_a = _fold(ctx, seqs, span, chunk, 1)
    b, chunks_b, dense_b, gen_b = _fold(ctx, seqs, span, chunk, 0)
    s, chunks_s, dense_s, gen_s = _fold(ctx, seqs, span, 0, -1)
    assert (chunks_a, chunks_b, chunks_s) == (chunks, chunks, 0)
    assert (dense_a, gen_a) == (dense_s, gen_s) and (dense_b, gen_b) == (dense_s, gen_s)
    _same(a, s, len(seqs))
    _same(b, s, len(seqs))
    return a, dense_a, gen_a


@pytest.fixture(scope="module")
def overflow(gpu_ctx):
    """the tandem repeats whose candidate pool does overflow (each folded alone on the serial path), shortest first"""
    over = sorted((s for s in TANDEM if _fold(gpu_ctx, [s], 300, 0, -1)[2] == 1), key=len)
    assert len(over) >= 6
    return over


def test_fourteen_chunks_of_mixed_lengths(gpu_ctx):
    """876 windows of length 5..350 at chunk 64: 14 chunks, so every pairing of fill stream (k mod 2) and slot (k mod 3) is used at least twice; the
    last chunk holds 44 windows."""
    seqs = seqgen.windows(10256, 876, 5, 350)
    a, _, _ = _three(gpu_ctx, seqs, 300, 64, 14)
    _oracle(seqs, 300, a, list(range(0, 832, 8)) + list(range(832, 876)))


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunks_of_one_and_two_windows(gpu_ctx, chunk):
    """40 windows of 5..40 nt: the fills end almost at once, grids of several chunks are in flight and leave and enter on every CU."""
    seqs = seqgen.windows(10257, 40, 5, 40)
    a, _, _ = _three(gpu_ctx, seqs, 300, chunk, 40 // chunk)
    _oracle(seqs, 300, a, list(range(40)))


@pytest.mark.parametrize("where", ["first", "last", "every", "whole_chunk"])
def test_pool_overflow_windows(gpu_ctx, overflow, where):
    """Five chunks of 32 windows with tandem repeats (pool overflow: the deferred dense pass and a second epilogue over the chunk) only in the first
    chunk, only in the last, in every chunk, and one chunk made of nothing else."""
    r = random.Random(len(where))
    seqs = seqgen.windows(10258, 5 * 32, 30, 350)
    put = {"first": [0], "last": [4], "every": [0, 1, 2, 3, 4], "whole_chunk": []}[where]
    n_over = 0
    for c in put:
        for k, w in enumerate(r.sample(range(32 * c, 32 * c + 32), 3)):
            seqs[w] = overflow[(k + c) % len(overflow)]
            n_over += 1
    if where == "whole_chunk":
        seqs[64:96] = [overflow[k % len(overflow)] for k in range(32)]
        n_over = 32
    a, n_dense, _ = _three(gpu_ctx, seqs, 300, 32, 5)
    assert n_dense >= n_over >= 1
    if where == "every":
        which = [w for w in range(len(seqs)) if int(a["status"][w]) == 0]
        _oracle(seqs, 300, a, which[::2])


def test_gc_windows_outside_16_bits_in_several_chunks(gpu_ctx, overflow):
    """GC-rich windows whose energies leave the 16-bit range go to the generic kernel from chunks 0, 2, 3 and 5, next to pool-overflow windows; a window
    that a dense pass hands on to the generic kernel is put into chunk 4 if the families hold one (the fallback count is read behind the deferred passes)."""
    alone = {s: _fold(gpu_ctx, [s], 300, 0, -1)[2:] for s in GC + TANDEM}
    handed_on = [s for s, (dense, gen) in alone.items() if dense == 1 and gen == 1]
    print("windows handed on by the dense pass to the generic kernel: %d" % len(handed_on))
    seqs = seqgen.windows(10259, 6 * 32, 30, 350)
    for c, at in ((0, 3), (2, 17), (3, 0), (5, 31)):
        seqs[32 * c + at] = GC[c % len(GC)]
        seqs[32 * c + (at + 7) % 32] = overflow[c % len(overflow)]
    for k, s in enumerate(handed_on[:4]):
        seqs[32 * 4 + 5 * k] = s
    a, n_dense, n_generic = _three(gpu_ctx, seqs, 300, 32, 6)
    assert n_dense >= 4 and n_generic >= 1
    which = [w for w in range(len(seqs)) if int(a["status"][w]) == 0]
    _oracle(seqs, 300, a, which[::3])


def test_calls_back_to_back_big_small_big(gpu_ctx, overflow):
    """Big with dense windows (nine chunks), small without (two), big again: per-chunk counters and dense lists of an earlier call must not be seen."""
    big = seqgen.windows(10260, 280, 20, 350)
    for w in (5, 100, 279):
        big[w] = overflow[w % len(overflow)]
    small = seqgen.windows(10261, 40, 20, 200)
    want_big, _, dense_big, gen_big = _fold(gpu_ctx, big, 300, 0, -1)
    want_small, _, dense_small, gen_small = _fold(gpu_ctx, small, 300, 0, -1)
    assert dense_big >= 3 and dense_small == 0
    for seqs, want, dense, gen, chunks in ((big, want_big, dense_big, gen_big, 9), (small, want_small, 0, gen_small, 2), (big, want_big, dense_big, gen_big, 9)):
        got, n_chunks, n_dense, n_gen = _fold(gpu_ctx, seqs, 300, 32, 1)
        assert (n_chunks, n_dense, n_gen) == (chunks, dense, gen)
        _same(got, want, len(seqs))
    _oracle(big, 300, got, list(range(0, 280, 7)))


def test_paths_that_stay_serial(gpu_ctx):
    """vienna-1.8.5, the dense split path and an automatic batch below the threshold with the tail-free schedule requested: no chunks, equal results."""
    seqs = seqgen.windows(10262, 120, 5, 350) + TANDEM[:2]
    try:
        gpu_ctx.set_fold_model("vienna-1.8.5")
        a, chunks_a, _, _ = _fold(gpu_ctx, seqs, 300, 32, 1)
        b, _, _, _ = _fold(gpu_ctx, seqs, 300, 0, -1)
    finally:
        gpu_ctx.set_fold_model("vienna-2.1.2")
    assert chunks_a == 0
    _same(a, b, len(seqs))
    _oracle(seqs, 300, a, list(range(0, 120, 4)), model="vienna-1.8.5")
    b, _, dense_b, gen_b = _fold(gpu_ctx, seqs, 300, 0, -1)
    try:
        gpu_ctx.set_fold_split_path(1)
        a, chunks_a, dense_a, gen_a = _fold(gpu_ctx, seqs, 300, 32, 1)
    finally:
        gpu_ctx.set_fold_split_path(0)
    assert chunks_a == 0 and dense_a == 0 and gen_a == gen_b
    _same(a, b, len(seqs))
    a, chunks_a, dense_a, gen_a = _fold(gpu_ctx, seqs, 300, -1, 1)      # automatic: 122 windows are far below 8 rounds of the fill grid
    assert chunks_a == 0 and (dense_a, gen_a) == (dense_b, gen_b)
    _same(a, b, len(seqs))


def test_kernel_times_of_a_tailfree_fold(gpu_ctx):
    """last_fold_kernel_ms() after a tail-free fold with deferred dense passes: both numbers >= 0, their sum no more than the call's wall time."""
    seqs = seqgen.windows(10263, 200, 100, 350)
    seqs[150] = TANDEM[0]
    gpu_ctx.fold_batch_raw(seqs[:8], 300, 96)
    try:
        gpu_ctx.set_fold_overlap(32)
        gpu_ctx.set_fold_overlap_tailfree(1)
        t = time.perf_counter()
        gpu_ctx.fold_batch_raw(seqs, 300, 96)
        wall_ms = 1e3 * (time.perf_counter() - t)
        chunks = gpu_ctx.last_fold_overlap_chunks()
        fill_ms, rest_ms = gpu_ctx.last_fold_kernel_ms()
    finally:
        gpu_ctx.set_fold_overlap(-1)
        gpu_ctx.set_fold_overlap_tailfree(-1)
    assert chunks == 7
    assert fill_ms >= 0 and rest_ms >= 0 and fill_ms + rest_ms > 0
    assert fill_ms + rest_ms <= wall_ms, (fill_ms, rest_ms, wall_ms)

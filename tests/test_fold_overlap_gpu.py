"""GPU parity of the chunked fold (set_fold_overlap: the epilogue of a chunk of windows on a second stream beside the fill of the next chunk, slab
slots, window states, dense lists and work counters reused from chunk to chunk) against the serial path (set_fold_overlap(0)) and the CPU oracle.
Equality with the serial path is exact: line count, every line (text, energy, start column, printed flag), MFE and status of every window, and the
numbers of windows handed to the dense fill kernel and to the generic kernel.  Small chunk overrides make tiny batches run many chunks."""
import random

import numpy as np
import pytest

from tests import seqgen
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu

TANDEM = [(u * 350)[:n] for u in ("AU", "GU", "AAUU", "ACGU", "GGGUUC", "AGU") for n in (350, 349, 301, 256)]      # pool overflow: the dense fill kernel
GC = ["G" * 150 + "C" * 150, "G" * 170 + "AAAA" + "C" * 170, "GC" * 150, "G" * 160 + "UUCG" + "C" * 160]          # energies outside 16 bits: the generic kernel


def _fold(ctx, seqs, span, overlap, max_lines=96):
    """(raw arrays, chunks, windows handed to the dense kernel, windows handed to the generic kernel) with the switch at `overlap`"""
    try:
        ctx.set_fold_overlap(overlap)
        raw = ctx.fold_batch_raw(seqs, span, max_lines)
        return raw, ctx.last_fold_overlap_chunks(), ctx.last_fold_dense(), ctx.last_fold_fallbacks()
    finally:
        ctx.set_fold_overlap(-1)


def _same(a, b, n, max_lines=96):
    for f in ("n_lines", "mfe", "status"):
        assert np.array_equal(a[f], b[f]), f
    assert len(a["n_lines"]) == n
    for w in range(n):
        nl = min(int(a["n_lines"][w]), max_lines)
        assert a["lines"][w, :nl].tobytes() == b["lines"][w, :nl].tobytes(), w
        for k in range(nl):
            ln = int(a["lines"][w, k]["len"])
            assert a["ss"][w, k, :ln].tobytes() == b["ss"][w, k, :ln].tobytes(), (w, k)


def _lines(raw, w, max_lines=96):
    out = []
    for k in range(min(int(raw["n_lines"][w]), max_lines)):
        ln = raw["lines"][w, k]
        if ln["printed"]:
            out.append((raw["ss"][w, k, :int(ln["len"])].tobytes().decode(), int(ln["energy"]), int(ln["start"])))
    return out


def _oracle(seqs, span, raw, which, model="vienna-2.1.2"):
    assert len(which) <= 150
    want = oracle_fold_all([seqs[w] for w in which], span, model)
    for w, (lines, mfe) in zip(which, want):
        assert int(raw["status"][w]) == 0, w
        assert (_lines(raw, w), int(raw["mfe"][w])) == (lines, mfe), (w, seqs[w])


def _both(ctx, seqs, span, chunk, chunks):
    a, n_chunks, dense_a, gen_a = _fold(ctx, seqs, span, chunk)
    b, n_serial, dense_b, gen_b = _fold(ctx, seqs, span, 0)
    assert n_chunks == chunks and n_serial == 0
    assert (dense_a, gen_a) == (dense_b, gen_b)
    _same(a, b, len(seqs))
    return a, dense_a, gen_a


def test_six_chunks_of_mixed_lengths(gpu_ctx):
    """1,300 windows of length 5..350 at chunk 256: six chunks, so every slab slot and counter block is used twice, and the last chunk holds 20 windows."""
    seqs = seqgen.windows(9256, 1300, 5, 350)
    a, _, _ = _both(gpu_ctx, seqs, 300, 256, 6)
    _oracle(seqs, 300, a, list(range(0, 1280, 10)) + list(range(1280, 1300)))


def test_hand_offs_outside_the_first_chunk(gpu_ctx):
    """Chunks of 64: an ordinary one, one made only of pool-overflow windows, then tandem repeats and GC windows scattered over four more.  The dense
    pass and the generic kernel must get exactly the windows they get on the serial path, whichever chunk and slot they come from."""
    r = random.Random(64)
    mixed = seqgen.windows(6401, 64 * 5, 40, 350)
    over = [s for s in TANDEM if _fold(gpu_ctx, [s], 300, 0)[2] == 1]      # the repeats whose pool does overflow (folded alone, serial path)
    assert len(over) >= 6
    seqs = mixed[:64] + [over[k % len(over)] for k in range(64)]
    for c in range(4):
        part = mixed[64 * (c + 1):64 * (c + 2)]
        for k, s in enumerate(TANDEM[6 * c:6 * c + 6] + GC):
            part[r.randrange(len(part))] = s
        seqs += part
    assert len(seqs) == 6 * 64
    a, n_dense, n_generic = _both(gpu_ctx, seqs, 300, 64, 6)
    assert n_dense >= 64 and n_generic >= 1
    which = [w for w in range(len(seqs)) if int(a["status"][w]) == 0]
    _oracle(seqs, 300, a, which[:40] + which[64:104:2] + which[-60:])


def test_batch_sizes_around_the_chunk(gpu_ctx):
    """1, chunk - 1, chunk, chunk + 1 and 2 x chunk + 1 windows at chunk 64."""
    seqs = seqgen.windows(6402, 129, 5, 350)
    for n, chunks in ((1, 1), (63, 1), (64, 1), (65, 2), (129, 3)):
        _both(gpu_ctx, seqs[:n], 300, 64, chunks)
    a, _, _, _ = _fold(gpu_ctx, seqs, 300, 64)
    _oracle(seqs, 300, a, list(range(129)))


def test_two_calls_back_to_back_reuse_events_counters_and_slots(gpu_ctx):
    """A fold of seven chunks, one of three, the first again: the second and third calls find the events, counter blocks, slots and the second stream of
    the calls before them."""
    big, small = seqgen.windows(6403, 400, 5, 350), seqgen.windows(6404, 150, 100, 350) + TANDEM[:3]
    want_big, _, dense_big, _ = _fold(gpu_ctx, big, 300, 0)
    want_small, _, dense_small, _ = _fold(gpu_ctx, small, 300, 0)
    assert dense_small >= 1
    for seqs, want, dense, chunks in ((big, want_big, dense_big, 7), (small, want_small, dense_small, 3), (big, want_big, dense_big, 7)):
        got, n_chunks, n_dense, _ = _fold(gpu_ctx, seqs, 300, 64)
        assert (n_chunks, n_dense) == (chunks, dense)
        _same(got, want, len(seqs))


def test_other_paths_stay_serial(gpu_ctx):
    """vienna-1.8.5 and the dense split path with overlap requested: the serial path, the same results."""
    seqs = seqgen.windows(6405, 200, 5, 350) + TANDEM[:2]
    try:
        gpu_ctx.set_fold_model("vienna-1.8.5")
        a, chunks_a, _, _ = _fold(gpu_ctx, seqs, 300, 64)
        b, _, _, _ = _fold(gpu_ctx, seqs, 300, 0)
    finally:
        gpu_ctx.set_fold_model("vienna-2.1.2")
    assert chunks_a == 0
    _same(a, b, len(seqs))
    _oracle(seqs, 300, a, list(range(0, 200, 4)), model="vienna-1.8.5")
    try:
        gpu_ctx.set_fold_split_path(1)
        a, chunks_a, dense_a, _ = _fold(gpu_ctx, seqs, 300, 64)
    finally:
        gpu_ctx.set_fold_split_path(0)
    b, _, _, _ = _fold(gpu_ctx, seqs, 300, 0)
    assert chunks_a == 0 and dense_a == 0
    _same(a, b, len(seqs))


def test_kernel_times_add_up_to_at_most_the_fold(gpu_ctx):
    """last_fold_kernel_ms() of a chunked fold: first fill's start to last fill's end, and the exposed rest; both >= 0, together no more than the fold
    stage's device time."""
    from mir_prefer_amd import synth
    ds = synth.make_dataset([60000, 40000], 40, n_samples=2, seed=3, contig_names=["chrB", "chrA"], edge_cases=True)
    order = np.argsort(np.array(ds.contig_names, dtype=object), kind="stable").astype(np.int32)
    gpu_ctx.load_genome(ds.contigs)
    gpu_ctx.load_alignments(ds.sorted_alns())
    _, _, nwin = gpu_ctx.candidate(10, 100, 300, order)
    assert nwin >= 3
    try:
        gpu_ctx.set_fold_overlap(max(1, nwin // 3))
        gpu_ctx.fold(300)
        chunks = gpu_ctx.last_fold_overlap_chunks()
        fill_ms, rest_ms = gpu_ctx.last_fold_kernel_ms()
        fold_ms = gpu_ctx.last_timings()["fold_ms"]
    finally:
        gpu_ctx.set_fold_overlap(-1)
    assert chunks >= 3
    assert fill_ms >= 0 and rest_ms >= 0 and fill_ms + rest_ms > 0
    assert fill_ms + rest_ms <= fold_ms, (fill_ms, rest_ms, fold_ms)

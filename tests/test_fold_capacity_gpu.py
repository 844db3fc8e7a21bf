"""GPU tests of the fold's capacity bound (set_fold_capacity: at most N windows' slabs resident).  Lowered, it makes small batches take the paths
that only a batch of more than 8 GiB of slabs takes otherwise: several serial sub-batches (counters cleared between them, the dense and fallback
totals and the kernel times accumulated over them) and ring slots of the chunked fold that hold N / 3 windows.  Every result is compared exactly
(_same of test_fold_overlap_gpu.py, last_fold_dense() and last_fold_fallbacks()) with the serial path at the default capacity, which is also checked
against the CPU oracle."""
import time

import pytest

from tests import seqgen
from tests.test_fold_overlap_gpu import GC, TANDEM, _lines, _same
from tests.test_whole_workload_gpu import oracle_fold_all

pytestmark = pytest.mark.gpu

SPAN = 300
CASES = {"default": ("vienna-2.1.2", 0), "default-dense": ("vienna-2.1.2", 1), "v185": ("vienna-1.8.5", 0), "v185-dense": ("vienna-1.8.5", 1)}


def _fold(ctx, seqs, capacity, overlap=0, tailfree=-1, model="vienna-2.1.2", split=0):
    """(raw arrays, chunks, windows handed to the dense kernel, windows handed to the generic kernel); every switch is put back"""
    try:
        ctx.set_fold_model(model)
        ctx.set_fold_split_path(split)
        ctx.set_fold_overlap(overlap)
        ctx.set_fold_overlap_tailfree(tailfree)
        ctx.set_fold_capacity(capacity)
        raw = ctx.fold_batch_raw(seqs, SPAN, 96)
        return raw, ctx.last_fold_overlap_chunks(), ctx.last_fold_dense(), ctx.last_fold_fallbacks()
    finally:
        ctx.set_fold_capacity(0)
        ctx.set_fold_overlap_tailfree(-1)
        ctx.set_fold_overlap(-1)
        ctx.set_fold_split_path(0)
        ctx.set_fold_model("vienna-2.1.2")


@pytest.fixture(scope="module")
def overflow(gpu_ctx):
    """the tandem repeats whose candidate pool does overflow (each folded alone on the serial path), shortest first"""
    over = sorted((s for s in TANDEM if _fold(gpu_ctx, [s], 0)[2] == 1), key=len)
    assert len(over) >= 6
    return over


@pytest.fixture(scope="module")
def forty(overflow):
    """40 short windows; at capacity 7 the sub-batches are [0, 7), [7, 14), ... [35, 40): pool-overflow windows in the first and the last one, a window
    for the generic kernel in the third"""
    seqs = seqgen.windows(11256, 40, 5, 120)
    seqs[3], seqs[16], seqs[37] = overflow[0], GC[0], overflow[1]
    assert len({3 // 7, 16 // 7, 37 // 7}) == 3 and 37 // 7 == (40 - 1) // 7
    return seqs


@pytest.fixture(scope="module")
def serial_at_default(gpu_ctx, forty):
    """case -> the serial fold of `forty` at capacity 0, every window of status 0 checked against the CPU oracle (one oracle fold per model)"""
    want = {model: oracle_fold_all(forty, SPAN, model) for model in sorted({m for m, _ in CASES.values()})}
    out = {}
    for case, (model, split) in CASES.items():
        raw, chunks, dense, generic = out[case] = _fold(gpu_ctx, forty, 0, model=model, split=split)
        assert chunks == 0
        ok = [w for w in range(len(forty)) if int(raw["status"][w]) == 0]
        assert len(ok) <= 150
        for w in ok:
            assert (_lines(raw, w), int(raw["mfe"][w])) == want[model][w], (case, w, forty[w])
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_serial_sub_batches(gpu_ctx, forty, serial_at_default, case):
    """Capacities 1, 7, 39 and 40: 40, 6, 2 and 1 sub-batches give what the one sub-batch of the default capacity gives."""
    model, split = CASES[case]
    want, _, dense, generic = serial_at_default[case]
    print("%s: %d windows to the dense kernel, %d to the generic kernel" % (case, dense, generic))
    if case == "default":
        assert dense >= 2 and generic >= 1
    for capacity in (1, 7, 39, 40):
        got, chunks, n_dense, n_generic = _fold(gpu_ctx, forty, capacity, model=model, split=split)
        assert chunks == 0
        assert (n_dense, n_generic) == (dense, generic), capacity
        _same(got, want, len(forty))


@pytest.fixture(scope="module")
def ninety_five(gpu_ctx, overflow):
    seqs = seqgen.windows(11257, 95, 5, 120)
    seqs[23], seqs[92] = overflow[2], GC[1]
    return seqs, _fold(gpu_ctx, seqs, 0)


@pytest.mark.parametrize("tailfree", [1, 0])
@pytest.mark.parametrize("capacity,chunks", [(30, 10), (3, 95), (2, 95)])
def test_ring_slots_bounded_by_the_capacity(gpu_ctx, ninety_five, capacity, chunks, tailfree):
    """95 windows with chunks of 64 requested: a slot of the ring holds a third of the capacity, so 30 gives chunks of 10 (the last one of 5) and
    3 and 2 give chunks of one window."""
    seqs, (want, serial_chunks, dense, generic) = ninety_five
    assert serial_chunks == 0 and dense >= 1 and generic >= 1
    got, n_chunks, n_dense, n_generic = _fold(gpu_ctx, seqs, capacity, overlap=64, tailfree=tailfree)
    assert n_chunks == chunks
    assert (n_dense, n_generic) == (dense, generic)
    _same(got, want, len(seqs))


def test_setter_validation(gpu_ctx, forty, serial_at_default):
    from mir_prefer_amd import capi
    with pytest.raises(capi.MirpError):
        gpu_ctx.set_fold_capacity(-1)
    want, chunks, dense, generic = serial_at_default["default"]
    try:
        gpu_ctx.set_fold_capacity(7)
        gpu_ctx.set_fold_capacity(0)
        gpu_ctx.set_fold_overlap(0)
        got = gpu_ctx.fold_batch_raw(forty, SPAN, 96)
        assert (gpu_ctx.last_fold_overlap_chunks(), gpu_ctx.last_fold_dense(), gpu_ctx.last_fold_fallbacks()) == (chunks, dense, generic)
    finally:
        gpu_ctx.set_fold_capacity(0)
        gpu_ctx.set_fold_overlap(-1)
    _same(got, want, len(forty))


def test_kernel_times_over_sub_batches(gpu_ctx, forty):
    """last_fold_kernel_ms() of a serial fold in six sub-batches: both numbers >= 0, their sum > 0 and no more than the call's wall time."""
    try:
        gpu_ctx.set_fold_overlap(0)
        gpu_ctx.set_fold_capacity(7)
        t = time.perf_counter()
        gpu_ctx.fold_batch_raw(forty, SPAN, 96)
        wall_ms = 1e3 * (time.perf_counter() - t)
        chunks = gpu_ctx.last_fold_overlap_chunks()
        fill_ms, epi_ms = gpu_ctx.last_fold_kernel_ms()
    finally:
        gpu_ctx.set_fold_capacity(0)
        gpu_ctx.set_fold_overlap(-1)
    assert chunks == 0
    assert fill_ms >= 0 and epi_ms >= 0 and fill_ms + epi_ms > 0
    assert fill_ms + epi_ms <= wall_ms, (fill_ms, epi_ms, wall_ms)

// mirp_run_fold: the host driver of the fold.  A short dispatcher over the generic fallback (tables in a global workspace), the serial
// path and the chunked path of the LDS-resident kernels (fold_lds_kernel.hip) with the deferred dense passes of its tail-free schedule, and the
// diagnostics of a -DMIRP_DIAG build.  The control block the kernels count in is named in fold_ctl.h, the chunk plan and the ring in fold_overlap_plan.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "fold_ctl.h"
#include "fold_overlap_plan.h"

namespace {

#define FOLD_LAUNCH(c, call)                                                                                                      \
    do {                                                                                                                          \
        hipError_t e_ = (call);                                                                                                   \
        if (e_ != hipSuccess) return fail((c), -2, std::string("fold LDS kernel launch failed: ") + hipGetErrorString(e_));       \
    } while (0)

// Diagnostics exist only in a -DMIRP_DIAG build (`make DIAG=1`, profiles/tools/): MIRP_FOLD_CLOCKS=1 prints phase clocks (=2: light mode, per wave only
// busy time, reported as splits, and barrier wait; the epilogue's clocks print with the fill's), MIRP_FOLD_DUMP=<path> dumps slabs,
// MIRP_FOLD_OVERLAP_TRACE prints when each kernel of a chunked fold ended, MIRP_FOLD_OVERLAP / MIRP_FOLD_TAILFREE set the switches for tools that
// cannot call them.  The shipped library reads no environment.
struct FoldDiag { int clocks = 0; bool trace = false; const char* dump = nullptr; };

// One call of mirp_run_fold: its arguments, and what the paths share
struct FoldCall {
    mirp_ctx* c; const unsigned char* seqs; const long long* offs; const int* lens; int n_work, n_cap, span, max_lines, stride;
    MirpFoldLine* lines; char* ss; int* nlines; int* mfe; int* status;
    bool m185; size_t slab; unsigned int* ctl; FoldDiag diag;
    // the launch arguments of windows [b0, b0 + nb): their slabs and window states from window `at` of the archive on, control block `block`
    mirp::FoldLdsArgs args(int b0, int nb, size_t at, int block, int* dense_list) const {
        return {m185 ? c->d_params185l : c->d_params, seqs, offs + b0, lens ? lens + b0 : nullptr, nb, b0, span, (short*)c->carch.p + at * 3 * slab, slab, (int*)c->wstate.p + at,
                ctl + mirp::FOLD_CTL_BLOCK * block, (int*)c->flist.p, ctl + mirp::FOLD_CTL_FALLBACKS, lines + (size_t)b0 * max_lines, ss + (size_t)b0 * max_lines * stride,
                nlines + b0, mfe + b0, status + b0, max_lines, stride, dense_list, 0, nullptr};
    }
};

// The fold's events: one pool in the context, grown on demand; a path names the ones it uses.
int fold_events(mirp_ctx* c, size_t n, hipEvent_t** ev) {
    while (c->fold_ev.size() < n) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); c->fold_ev.push_back(e); }
    *ev = c->fold_ev.data();
    return 0;
}
struct SerialEvents {      // per sub-batch: around its fill and its epilogue
    hipEvent_t* ev;
    static size_t count(int n_sub) { return 3 * (size_t)n_sub; }
    hipEvent_t fill_starts(int k) const { return ev[3 * k]; }
    hipEvent_t fill_done(int k) const { return ev[3 * k + 1]; }
    hipEvent_t epilogue_done(int k) const { return ev[3 * k + 2]; }
};
struct ChunkEvents {       // of the call, then per chunk
    hipEvent_t* ev;
    static size_t count(int n_chunks) { return 4 + 2 * (size_t)n_chunks; }
    hipEvent_t first_fill_starts() const { return ev[0]; }
    hipEvent_t all_done() const { return ev[1]; }
    hipEvent_t deferred_start() const { return ev[2]; }
    hipEvent_t deferred_done() const { return ev[3]; }
    hipEvent_t fill_done(int k) const { return ev[4 + 2 * k]; }
    hipEvent_t epilogue_done(int k) const { return ev[5 + 2 * k]; }
};

#ifdef MIRP_DIAG
FoldDiag read_diag(mirp_ctx* c) {
    FoldDiag d;
    if (const char* ov = std::getenv("MIRP_FOLD_OVERLAP")) c->fold_overlap = std::atoi(ov);
    if (const char* tf = std::getenv("MIRP_FOLD_TAILFREE")) c->fold_tailfree = std::atoi(tf);
    if (const char* clk = std::getenv("MIRP_FOLD_CLOCKS")) d.clocks = std::atoi(clk) == 2 ? 2 : 1;
    d.trace = std::getenv("MIRP_FOLD_OVERLAP_TRACE") != nullptr;
    d.dump = std::getenv("MIRP_FOLD_DUMP");
    return d;
}
int print_clocks(const FoldCall& f) {
    long long cyc[mirp::FOLD_CTL_CLOCKS_N];
    HIPCHK(f.c, hipMemcpy(cyc, f.ctl + mirp::FOLD_CTL_CLOCKS, sizeof(cyc), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[mirp fold clocks] windows=%d setup=%lld fillA=%lld fillB=%lld writeout=%lld (sum over workgroups, s_memtime ticks)\n", f.n_work, cyc[0], cyc[1], cyc[2], cyc[3]);
    for (int w = 0; w < 16; w++)
        std::fprintf(stderr, "[mirp fold clocks] wave %2d: phaseB=%lld interior=%lld splits=%lld barrier=%lld\n", w, cyc[4 + 4 * w], cyc[5 + 4 * w], cyc[6 + 4 * w], cyc[7 + 4 * w]);
    for (int b = 0; b < 4; b++)
        std::fprintf(stderr, "[mirp fold clocks] wave 9, diagonals with %d%s blocks: %lld, interior ticks %lld\n", b, b == 3 ? "+" : "", cyc[72 + b], cyc[68 + b]);
    std::fprintf(stderr, "[mirp fold clocks] ramp-up intervals (interior loops with um < MAXLOOP): %lld of %lld intervals, %lld of fillB=%lld ticks (%.1f %%)\n", cyc[77], cyc[78],
                 cyc[76], cyc[2], cyc[2] ? 100.0 * (double)cyc[76] / (double)cyc[2] : 0.0);
    for (int b = 0; b < 8; b++)      // thread 0's barrier intervals by the blocks of paired cells their interior loops ran: the fixed part and the part per block
        std::fprintf(stderr, "[mirp fold clocks] %s intervals with %d%s blocks: %lld, thread 0 ticks %lld\n", b < 4 ? "steady-state" : "ramp-up", b & 3, (b & 3) == 3 ? "+" : "",
                     cyc[87 + b], cyc[79 + b]);
    mirp::fold_lds_epi_clocks_print();
    return 0;
}
int dump_slab(const FoldCall& f) {      // c / fML / trace-back slabs of the first window of the last sub-batch
    std::vector<short> h(3 * f.slab);
    HIPCHK(f.c, hipMemcpy(h.data(), f.c->carch.p, 6 * f.slab, hipMemcpyDeviceToHost));
    if (FILE* out = std::fopen(f.diag.dump, "wb")) { std::fwrite(h.data(), 2, h.size(), out); std::fclose(out); }
    return 0;
}
#else
FoldDiag read_diag(mirp_ctx*) { return FoldDiag(); }
int print_clocks(const FoldCall&) { return 0; }
int dump_slab(const FoldCall&) { return 0; }
#endif

// Fold dedup (mirp_fold, fold_dedup_kernels.hip): the duplicates have length 0 and are on no hand-off list, so a list's windows count with their
// duplicates (c->dup_run.n_dup, null for every other caller: nothing below launches then).  The sums go to words of block 0 and reach the host with it.
int count_dense_dups(const FoldCall& f, hipStream_t st, const int* dense_list, int block, int b0) {      // behind a dense pass over the list of `block`
    if (!f.c->dup_run.n_dup) return 0;
    FOLD_LAUNCH(f.c, mirp::launch_fold_dedup_count(st, dense_list, f.ctl + mirp::FOLD_CTL_BLOCK * block + mirp::FOLD_CTL_DENSE_LEN, b0, f.c->dup_run.n_dup,
                                                   f.ctl + mirp::FOLD_CTL_DUP_DENSE, true, nullptr, nullptr));
    return 0;
}
int count_fallback_dups(const FoldCall& f) {      // in front of a read-back of block 0, every fill done: the whole fallback list, and the call's duplicate count
    if (!f.c->dup_run.n_dup) return 0;
    FOLD_LAUNCH(f.c, mirp::launch_fold_dedup_count(f.c->stream, (const int*)f.c->flist.p, f.ctl + mirp::FOLD_CTL_FALLBACKS, 0, f.c->dup_run.n_dup,
                                                   f.ctl + mirp::FOLD_CTL_DUP_FALLBACKS, false, f.c->dup_run.total, f.ctl + mirp::FOLD_CTL_DUPLICATES));
    return 0;
}
void read_dup_counts(mirp_ctx* c, const unsigned int* block0) {
    if (!c->dup_run.n_dup) return;
    c->dup_run.fallbacks = block0[mirp::FOLD_CTL_DUP_FALLBACKS]; c->dup_run.dense = block0[mirp::FOLD_CTL_DUP_DENSE]; c->dup_run.duplicates = block0[mirp::FOLD_CTL_DUPLICATES];
}

// Generic kernels (tables in a global workspace): every window when the LDS-resident path does not apply, else the windows it flagged.  A batch
// of `slots` windows (fill kernel, then epilogue kernel) at a time; the device may be shared: fewer windows per batch before giving up.
int run_generic(const FoldCall& f, const int* work_list, int n_generic) {
    mirp_ctx* c = f.c;
    if (f.m185 && mirp::fold185_lds_bytes(f.n_cap, f.max_lines) > 160 * 1024) return fail(c, -5, "LDS budget exceeded (vienna-1.8.5 kernel: window or max_lines too large)");
    // c, fML, DML ring, split-candidate pool of one window (PRECURSOR_LEN = 3000: 160 MB).  96 windows per CU and batch -- the hardware keeps as many
    // resident as registers and LDS allow: 6 of the fill, 8 of the epilogue -- make one batch of 20,000 windows: every batch ends with a tail of idle CUs
    // (three batches of 8,192: 0.075 s at L = 301, one: 0.069), and 288 GB hold the 45 - 75 GB
    const size_t slot_ints = f.m185 ? mirp::fold185_ws_slot_ints(f.n_cap, f.span) : mirp::fold_generic_ws_slot_ints(f.n_cap, f.span);
    int slots = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->n_cu * 96, ((size_t)128 << 30) / (slot_ints * 4)));
    slots = std::min(slots, n_generic);
    while (c->ws.ensure((size_t)slots * slot_ints * 4)) {
        if (slots <= 1) return fail(c, -6, "device allocation failed (fold workspace)");
        slots = (slots + 1) / 2; (void)hipGetLastError();
    }
    if (f.m185) {
        const hipError_t e = mirp::launch_fold185(c->stream, slots, c->d_params185, f.seqs, f.offs, f.lens, work_list, n_generic, f.span, f.n_cap, (int*)c->ws.p, slot_ints,
                                                  f.max_lines, f.stride, f.lines, f.ss, f.nlines, f.mfe, f.status);
        if (e != hipSuccess) return fail(c, -2, std::string("fold (vienna-1.8.5) kernel launch failed: ") + hipGetErrorString(e));
        return 0;
    }
    mirp::launch_fold_generic(c->stream, slots, c->d_params, f.seqs, f.offs, f.lens, work_list, n_generic, f.span, f.n_cap, (int*)c->ws.p, slot_ints, f.max_lines, f.stride,
                              f.lines, f.ss, f.nlines, f.mfe, f.status);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Serial path: sub-batches of at most `sub` windows, one behind the other on the context's stream and in the same slabs: a fill (default model: two
// 512-thread workgroups per CU; dense pass and vienna-1.8.5: one of 1024; tables in LDS), then an epilogue of many small workgroups; the two
// exchange the c / fML triangles of every window through per-window slabs in HBM.  All of them count in block 0 of the control block.
int run_serial(const FoldCall& f, int sub) {
    mirp_ctx* c = f.c;
    const int model = f.m185 ? 1 : 0, n_sub = (f.n_work + sub - 1) / sub;
    if (c->carch.ensure((size_t)sub * f.slab * 6) || c->wstate.ensure(4 * (size_t)sub) || c->dlist.ensure(4 * (size_t)sub))
        return fail(c, -6, "device allocation failed (fold LDS kernel)");
    SerialEvents ev;
    if (int rc = fold_events(c, SerialEvents::count(n_sub), &ev.ev)) return rc;
    for (int k = 0, b0 = 0; k < n_sub; k++, b0 += sub) {
        const int nb = std::min(sub, f.n_work - b0), grid = std::min(nb, c->n_cu);
        // the work counters and the dense list's length start again; the fallback count and the dense total keep accumulating
        if (k > 0) HIPCHK(c, hipMemsetAsync(f.ctl, 0, 4 * (mirp::FOLD_CTL_DENSE_LEN + 1), c->stream));
        mirp::FoldLdsArgs a = f.args(b0, nb, 0, 0, (int*)c->dlist.p);
        if (f.diag.clocks) { a.light_clocks = f.diag.clocks == 2; a.dbg_cycles = (long long*)(f.ctl + mirp::FOLD_CTL_CLOCKS); }
        HIPCHK(c, hipEventRecord(ev.fill_starts(k), c->stream));
        if (!c->fold_dense) FOLD_LAUNCH(c, mirp::launch_fold_lds_pool(c->stream, model, grid, a));
        FOLD_LAUNCH(c, mirp::launch_fold_lds_dense(c->stream, model, grid, a, c->fold_dense != 0));
        HIPCHK(c, hipEventRecord(ev.fill_done(k), c->stream));
        FOLD_LAUNCH(c, mirp::launch_fold_lds_epilogue(c->stream, model, std::min(nb, c->n_cu * 8), a));
        HIPCHK(c, hipEventRecord(ev.epilogue_done(k), c->stream));
        if (int rc = count_dense_dups(f, c->stream, (const int*)c->dlist.p, 0, b0)) return rc;
    }
    if (int rc = count_fallback_dups(f)) return rc;
    unsigned int h[mirp::FOLD_CTL_DUPLICATES + 1];
    HIPCHK(c, hipMemcpyAsync(h, f.ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_fallback = h[mirp::FOLD_CTL_FALLBACKS];
    c->last_dense = h[mirp::FOLD_CTL_DENSE_TOTAL];
    read_dup_counts(c, h);
    c->fold_kernel_ms[0] = c->fold_kernel_ms[1] = 0;
    for (int k = 0; k < n_sub; k++) {
        float fill = 0, epi = 0;
        (void)hipEventElapsedTime(&fill, ev.fill_starts(k), ev.fill_done(k));
        (void)hipEventElapsedTime(&epi, ev.fill_done(k), ev.epilogue_done(k));
        c->fold_kernel_ms[0] += fill; c->fold_kernel_ms[1] += epi;
    }
    if (f.diag.trace) std::fprintf(stderr, "[mirp fold overlap] serial path, largest pool fill %u entries\n", h[mirp::FOLD_CTL_POOL_MAX]);
    if (f.diag.dump) if (int rc = dump_slab(f)) return rc;
    if (f.diag.clocks) if (int rc = print_clocks(f)) return rc;
    return 0;
}

// The windows the pool passes of a tail-free fold handed to the dense pass (n_dense[k] of chunk k; none on the benchmark inputs), chunk by chunk on
// the context's stream, which has the device alone by now: the chunk's window states cleared, so that its second epilogue does nothing but them, the
// dense pass into the chunk's own slot, the epilogue.  A dense pass may hand windows on to the generic kernel: the fallback count is read again.
int run_deferred_dense(const FoldCall& f, const std::vector<int>& plan, const mirp::FoldRing& ring, const std::vector<unsigned int>& n_dense, const ChunkEvents& ev, float* ms) {
    mirp_ctx* c = f.c;
    HIPCHK(c, hipEventRecord(ev.deferred_start(), c->stream));
    for (int k = 0, b0 = 0; k < (int)plan.size(); b0 += plan[k], k++) {
        if (n_dense[k] == 0) continue;
        const mirp::FoldLdsArgs a = f.args(b0, plan[k], ring.at[k % mirp::FOLD_RING_SLOTS], 1 + k, (int*)c->dlist.p + b0);
        HIPCHK(c, hipMemsetAsync(a.win_state, 0, 4 * (size_t)plan[k], c->stream));
        HIPCHK(c, hipMemsetAsync(a.ctl + mirp::FOLD_CTL_EPILOGUE, 0, 4, c->stream));
        FOLD_LAUNCH(c, mirp::launch_fold_lds_dense(c->stream, 0, std::min(plan[k], c->n_cu), a, false));
        FOLD_LAUNCH(c, mirp::launch_fold_lds_epilogue(c->stream, 0, std::min(plan[k], c->n_cu * 8), a));
        if (int rc = count_dense_dups(f, c->stream, a.dense_list, 1 + k, b0)) return rc;
    }
    HIPCHK(c, hipEventRecord(ev.deferred_done(), c->stream));
    if (int rc = count_fallback_dups(f)) return rc;
    unsigned int h[mirp::FOLD_CTL_DUPLICATES + 1];      // block 0 from the fallback count on
    HIPCHK(c, hipMemcpyAsync(h + mirp::FOLD_CTL_FALLBACKS, f.ctl + mirp::FOLD_CTL_FALLBACKS, 4 * (mirp::FOLD_CTL_DUPLICATES + 1 - mirp::FOLD_CTL_FALLBACKS), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_fallback = h[mirp::FOLD_CTL_FALLBACKS];
    read_dup_counts(c, h);
    (void)hipEventElapsedTime(ms, ev.deferred_start(), ev.deferred_done());
    return 0;
}

// Chunked path ("fold overlap"; default model's candidate-pool pass only): the batch in the chunks of `plan`, the epilogue of chunk k on a stream of
// its own beside the fill of chunk k + 1.  The fill is an LDS / VALU kernel that moves 3 % of the HBM roof, the epilogue a chain of memory round trips
// with next to no arithmetic: the candidate-pool pass is built to leave room for MIRP_OVERLAP_EPI_WGS epilogue workgroups per CU
// (fold_lds_common.h).  The archive is a ring of FOLD_RING_SLOTS slots (slabs and window states of one chunk each, fold_overlap_plan.h); every chunk
// has a control block of its own behind the call's and its own stretch, at its first window, of one dense list of n_work entries, so nothing is
// cleared between chunks and the lists outlive the reuse of a slot.  One chunk touches: its fill stream, the epilogue stream, the events
// fill_done(k) and epilogue_done(k) (and epilogue_done(k - FOLD_RING_SLOTS), which frees its slot), control block 1 + k, and of block 0 the fallback
// count and the largest pool fill.
//
// Tail-free schedule (mirp_set_fold_overlap_tailfree, the default): fill k goes on stream k % 2 (the context's, stream_fill2) and does not wait for
// fill k - 1: both are persistent grids that draw windows from their own counters, and as workgroups of one run out of windows and exit, workgroups
// of the next take their places, so no CU idles at a chunk boundary.  The dense pass (1024 threads, 160 KB of LDS: it needs empty CUs) would drain
// them, so a chunk launches the candidate-pool pass only; a window it hands over keeps win_state 0, which the epilogue skips, and is folded behind
// the last epilogue (run_deferred_dense).  Ordered schedule (mode 0): every fill on the context's stream, pool pass and dense pass, as before round 10.
//
// Every dependency is an event, nothing polls memory: epilogue k waits for fill k, fill k for epilogue k - FOLD_RING_SLOTS, whose slot it takes
// over, and the second fill stream once for the event in front of the first fill (the counters' memset, the caller's uploads).  Every
// hipStreamWaitEvent below names an event recorded earlier in host submission order, so the schedule cannot deadlock even where two of the three
// streams share a hardware queue: it then only loses overlap.
int run_chunked(const FoldCall& f, const std::vector<int>& plan, bool tailfree) {
    mirp_ctx* c = f.c;
    const int n_chunks = (int)plan.size();
    const mirp::FoldRing ring = mirp::fold_overlap_ring(plan);
    if (c->carch.ensure((size_t)ring.windows() * f.slab * 6) || c->wstate.ensure(4 * (size_t)ring.windows()) || c->dlist.ensure(4 * (size_t)f.n_work))
        return fail(c, -6, "device allocation failed (fold LDS kernel)");
    if (!c->stream_epi) HIPCHK(c, hipStreamCreateWithFlags(&c->stream_epi, hipStreamNonBlocking));
    if (tailfree && !c->stream_fill2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream_fill2, hipStreamNonBlocking));
    ChunkEvents ev;
    if (int rc = fold_events(c, ChunkEvents::count(n_chunks), &ev.ev)) return rc;
    // what the two schedules answer differently: the stream of fill k, and whether the dense pass follows its pool pass or is deferred
    auto fill_stream = [&](int k) { return tailfree && (k & 1) ? c->stream_fill2 : c->stream; };
    const bool dense_per_chunk = !tailfree;
    HIPCHK(c, hipEventRecord(ev.first_fill_starts(), c->stream));
    if (tailfree) HIPCHK(c, hipStreamWaitEvent(c->stream_fill2, ev.first_fill_starts(), 0));
    for (int k = 0, b0 = 0; k < n_chunks; b0 += plan[k], k++) {
        const mirp::FoldLdsArgs a = f.args(b0, plan[k], ring.at[k % mirp::FOLD_RING_SLOTS], 1 + k, (int*)c->dlist.p + b0);
        const hipStream_t sf = fill_stream(k);
        const int grid = std::min(plan[k], c->n_cu);
        if (k >= mirp::FOLD_RING_SLOTS) HIPCHK(c, hipStreamWaitEvent(sf, ev.epilogue_done(k - mirp::FOLD_RING_SLOTS), 0));
        FOLD_LAUNCH(c, mirp::launch_fold_lds_pool(sf, 0, grid, a));
        if (dense_per_chunk) {
            FOLD_LAUNCH(c, mirp::launch_fold_lds_dense(sf, 0, grid, a, false));
            if (int rc = count_dense_dups(f, sf, a.dense_list, 1 + k, b0)) return rc;
        }
        HIPCHK(c, hipEventRecord(ev.fill_done(k), sf));
        HIPCHK(c, hipStreamWaitEvent(c->stream_epi, ev.fill_done(k), 0));
        // beside a fill: no more persistent epilogue workgroups than fit next to two fill workgroups on every CU; the last one has the device alone
        FOLD_LAUNCH(c, mirp::launch_fold_lds_epilogue(c->stream_epi, 0, std::min(plan[k], c->n_cu * (k + 1 < n_chunks ? c->overlap_epi_wgs : 8)), a));
        HIPCHK(c, hipEventRecord(ev.epilogue_done(k), c->stream_epi));
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, ev.epilogue_done(n_chunks - 1), 0));      // the epilogues are in order on their stream and each waits for its fill: the last one ends them all
    HIPCHK(c, hipEventRecord(ev.all_done(), c->stream));
    if (int rc = count_fallback_dups(f)) return rc;
    std::vector<unsigned int> h(mirp::FOLD_CTL_BLOCK * (size_t)(1 + n_chunks)), n_dense(n_chunks);
    HIPCHK(c, hipMemcpyAsync(h.data(), f.ctl, 4 * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_fallback = h[mirp::FOLD_CTL_FALLBACKS];
    c->last_dense = 0;
    for (int k = 0; k < n_chunks; k++) c->last_dense += n_dense[k] = h[mirp::FOLD_CTL_BLOCK * (1 + k) + mirp::FOLD_CTL_DENSE_LEN];
    c->last_overlap_chunks = n_chunks;
    read_dup_counts(c, h.data());
    float deferred_ms = 0;
    if (!dense_per_chunk && c->last_dense)
        if (int rc = run_deferred_dense(f, plan, ring, n_dense, ev, &deferred_ms)) return rc;
    // [0]: first fill's start to last fill's end, whichever stream it ends on (ordered schedule: dense passes included), [1]: the rest of the
    // fold's device time, i.e. the exposed epilogue and the deferred dense passes with their epilogues
    float fill_ms = 0, all_ms = 0;
    for (int k = 0; k < n_chunks; k++) {
        float t = 0;
        (void)hipEventElapsedTime(&t, ev.first_fill_starts(), ev.fill_done(k));
        fill_ms = std::max(fill_ms, t);
    }
    (void)hipEventElapsedTime(&all_ms, ev.first_fill_starts(), ev.all_done());
    c->fold_kernel_ms[0] = fill_ms; c->fold_kernel_ms[1] = std::max(0.0f, all_ms - fill_ms) + deferred_ms;
    if (f.diag.trace) {      // when each kernel ended, ms after the first fill's start
        for (int k = 0; k < n_chunks; k++) {
            float t = 0, e2 = 0;
            (void)hipEventElapsedTime(&t, ev.first_fill_starts(), ev.fill_done(k)); (void)hipEventElapsedTime(&e2, ev.first_fill_starts(), ev.epilogue_done(k));
            std::fprintf(stderr, "[mirp fold overlap] chunk %d: %d windows, fill done %.3f ms, epilogue done %.3f ms\n", k, plan[k], t, e2);
        }
        std::fprintf(stderr, "[mirp fold overlap] %s, all done %.3f ms, deferred dense %.3f ms, largest pool fill %u entries\n", tailfree ? "tail-free" : "ordered", all_ms,
                     deferred_ms, h[mirp::FOLD_CTL_POOL_MAX]);
    }
    return 0;
}

}  // namespace

int mirp_run_fold(mirp_ctx* c, const unsigned char* d_seqs, const long long* d_offs, const int* d_lens, int n_work, int n_cap, int span,
                  int max_lines, int stride, MirpFoldLine* d_lines, char* d_ss, int* d_nlines, int* d_mfe, int* d_status) {
    if (n_work <= 0) return 0;
    c->last_fallback = 0;
    c->last_overlap_chunks = 0;
    c->dup_run.fallbacks = c->dup_run.dense = 0; c->dup_run.duplicates = -1;
    FoldCall f = {c, d_seqs, d_offs, d_lens, n_work, n_cap, span, max_lines, stride, d_lines, d_ss, d_nlines, d_mfe, d_status, c->fold_model == MIRP_FOLD_MODEL_VIENNA_185, 0, nullptr, FoldDiag()};
    if (!f.m185 && mirp::fold_generic_lds_bytes(n_cap, max_lines) > 160 * 1024) return fail(c, -5, "LDS budget exceeded (window or max_lines too large)");
    // the generic kernel ranks interior-loop candidates by energy * 1024 + shape in 32 bits (fold_kernel.hip, GEN_EMAX): energies below 10^6 in magnitude
    if (!f.m185 && n_cap > 5000) return fail(c, -5, "window longer than 5,000 nt");
    if (span > mirp::fold_lds_max_span() || mirp::fold_lds_bytes(max_lines) > 160 * 1024) return run_generic(f, nullptr, n_work);
    f.diag = read_diag(c);
    if (c->fold_prepared_lines != max_lines) {      // first fold of the context, or another number of structure lines
        FOLD_LAUNCH(c, mirp::fold_lds_prepare(max_lines));
        c->overlap_epi_wgs = std::max(0, mirp::fold_lds_overlap_epi_wgs(max_lines));
        (void)hipGetLastError();
        c->fold_prepared_lines = max_lines;
    }
    // three 16-bit triangles per window: c, fML, trace-back codes.  At most 8 GiB of them are resident (mirp_set_fold_capacity: fewer), as one
    // sub-batch of the serial path or as the ring of the chunked path
    f.slab = mirp::fold_lds_slab_shorts(std::min(n_cap, mirp::fold_lds_max_n() + 2));
    const size_t resident = c->fold_cap > 0 ? (size_t)c->fold_cap : ~(size_t)0;
    const int sub = (int)std::max<size_t>(1, std::min(resident, std::min<size_t>((size_t)n_work, ((size_t)8 << 30) / (f.slab * 6))));
    // chunked: only the default model's candidate-pool pass, where a CU has room for an epilogue workgroup beside two of its workgroups; an empty plan: serial
    std::vector<int> plan;
    const bool tailfree = c->fold_tailfree != 0;
    if (!f.m185 && !c->fold_dense && c->fold_overlap != 0 && c->overlap_epi_wgs >= 1) {
        const size_t slot = std::max<size_t>(1, std::min(resident / mirp::FOLD_RING_SLOTS, ((size_t)8 << 30) / (f.slab * 6 * mirp::FOLD_RING_SLOTS)));
        plan = mirp::fold_overlap_plan(n_work, 2 * c->n_cu, (long long)slot, c->fold_overlap, tailfree ? mirp::FOLD_SCHEDULE_TAILFREE : mirp::FOLD_SCHEDULE_ORDERED);
    }
    const size_t ctl_bytes = std::max<size_t>(mirp::FOLD_CTL_MIN_BYTES, 4 * mirp::FOLD_CTL_BLOCK * (1 + plan.size()));
    if (c->fctl.ensure(ctl_bytes) || c->flist.ensure(4 * (size_t)n_work)) return fail(c, -6, "device allocation failed (fold LDS kernel)");
    f.ctl = (unsigned int*)c->fctl.p;
    HIPCHK(c, hipMemsetAsync(f.ctl, 0, ctl_bytes, c->stream));
    if (int rc = plan.empty() ? run_serial(f, sub) : run_chunked(f, plan, tailfree)) return rc;
    c->last_dense += (unsigned int)c->dup_run.dense;
    return c->last_fallback ? run_generic(f, (const int*)c->flist.p, (int)c->last_fallback) : 0;
}

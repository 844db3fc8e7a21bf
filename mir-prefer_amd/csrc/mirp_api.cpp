// C-ABI layer of libmirprefer.so (see include/mirprefer.h).  Host orchestration only: device
// buffers, streams, kernel launches.  There is NO CPU fallback: every entry point fails loudly
// if no gfx950 device / HIP runtime is usable.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mirp_internal.h"

#define MIRP_ABI_VERSION 17  // 17: mirp_duplex_batch, mirp_set_duplex_capacity, mirp_duplex_last_stats, MirpTargetOpts.energy; 16: mirp_randfold, mirp_shuffle_batch; 15: mirp_annotate_scan; 14: mirp_degradome_scan; 13: mirp_cluster_scan; 12: mirp_phase_scan; 11: mirp_target_scan, mirp_set_target_capacity; 10: mirp_trim_reads; 9: mirp_align_index, mirp_align_reads; 8: mirp_collapse_reads, mirp_last_collapse_collisions; 7: mirp_write_result_reports, mirp_fold_predict_report_stream, mirp_select_windows, mirp_dist_comm_info, MIRP_MAX_SAMPLES 255; 6: mirp_last_coverage_fused, mirp_fold_batch_summary, mirp_predict_batch_reasons, text writers; 5: mirp_dist_*, mirp_gather_loci / mirp_gather_records, mirp_read_fasta, mirp_ingest_sams_shard; 4: MirpSamData.segs, mirp_ingest_sams_gpu, mirp_load_coverage_segments; 2: mirp_set_fold_model, mirp_ingest_sams; 3: mirp_predict returns the per-window capacity status, mirp_get_fold_overflow
#define MIRP_NMAX 3096

#include "mirp_ctx.h"
#include "mirp_fasta.h"

extern "C" int mirp_abi_version(void) { return MIRP_ABI_VERSION; }

extern "C" void mirp_destroy(mirp_ctx* c);

extern "C" int mirp_create(int device, mirp_ctx** out) {
    if (!out) return -1;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -3;  // no GPU: fail loudly, no fallback
    if (device < 0 || device >= ndev) return -4;
    mirp_ctx* c = new mirp_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return -2; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return -2; }
    FoldParams* hp = new FoldParams();
    mirp_fill_fold_params(hp);
    if (hp->gen_wing_d != mirp::fold_lds_gen_wing_d()) {      // the fill kernel compiles this property of the table in (a1_gen_row_w)
        std::fprintf(stderr, "mirp_create: energy model and fill kernel disagree on the saturation of the asymmetry term (%d vs %d)\n", hp->gen_wing_d, mirp::fold_lds_gen_wing_d());
        delete hp; delete c; return -5;
    }
    if (hp->xb_bias < 0) { std::fprintf(stderr, "mirp_create: inner-pair terms outside the fill kernel's byte-table range\n"); delete hp; delete c; return -5; }
    for (int t = 1; t <= 6; t++)          // the fill kernel's list entries carry these two terms of a cell as 10-bit signed fields (fold_lds_kernel.hip, ENT_OUTER)
        for (int a = 0; a < 5; a++)
            for (int b = 0; b < 5; b++)
                if (hp->mismatchI[t][a][b] < -512 || hp->mismatchI[t][a][b] > 511 || hp->mismatch1nI[t][a][b] < -512 || hp->mismatch1nI[t][a][b] > 511) {
                    std::fprintf(stderr, "mirp_create: interior-loop mismatch energies outside the fill kernel's list-entry range\n");
                    delete hp; delete c; return -5;
                }
    if (hipMalloc((void**)&c->d_params, sizeof(FoldParams)) != hipSuccess ||
        hipMemcpy(c->d_params, hp, sizeof(FoldParams), hipMemcpyHostToDevice) != hipSuccess) {
        delete hp; delete c; return -2;
    }
    delete hp;
    for (int i = 0; i < 6; i++)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) { mirp_destroy(c); return -2; }
    *out = c;
    return 0;
}

// The piece in which text leaves the device (site_finish_pass of site_lines.h, mirp_download_text of mirp_ctx.h) and the pieces of the last call
extern "C" int mirp_set_text_piece(mirp_ctx* c, int64_t bytes) {
    if (!c) return -1;
    if (bytes < 0) return fail(c, -1, "mirp_set_text_piece: bad argument");
    c->text_piece = bytes;
    return 0;
}

extern "C" int64_t mirp_text_pieces_last(const mirp_ctx* c) { return c ? c->text_pieces : -1; }

// Launches and the largest jobs per resident slot of a wave-per-job kernel family in the last call that launches it (mirp_ctx::jobs_per_slot)
extern "C" int mirp_last_jobs_per_slot(mirp_ctx* c, int32_t family, int64_t out[2]) {
    if (!c) return -1;
    if (family < 0 || family > 8 || !out) return fail(c, -1, "mirp_last_jobs_per_slot: bad argument");
    out[0] = c->jobs_per_slot[family][0];
    out[1] = c->jobs_per_slot[family][1];
    return 0;
}

extern "C" int mirp_set_fold_model(mirp_ctx* c, int32_t model) {
    if (!c) return -1;
    if (model != MIRP_FOLD_MODEL_VIENNA_212 && model != MIRP_FOLD_MODEL_VIENNA_185) return fail(c, -1, "mirp_set_fold_model: unknown model");
    (void)hipSetDevice(c->device);
    if (model == MIRP_FOLD_MODEL_VIENNA_185 && !c->d_params185l) {
        FoldParams* hl = new FoldParams();
        mirp_fill_fold_params_t1999(hl);
        if (hipMalloc((void**)&c->d_params185l, sizeof(FoldParams)) != hipSuccess ||
            hipMemcpy(c->d_params185l, hl, sizeof(FoldParams), hipMemcpyHostToDevice) != hipSuccess) {
            delete hl;
            if (c->d_params185l) { (void)hipFree(c->d_params185l); c->d_params185l = nullptr; }
            return fail(c, -6, "mirp_set_fold_model: device allocation failed");
        }
        delete hl;
    }
    if (model == MIRP_FOLD_MODEL_VIENNA_185 && !c->d_params185) {
        FoldParams185* hp = new FoldParams185();
        mirp_fill_fold_params185(hp);
        if (hipMalloc((void**)&c->d_params185, sizeof(FoldParams185)) != hipSuccess ||
            hipMemcpy(c->d_params185, hp, sizeof(FoldParams185), hipMemcpyHostToDevice) != hipSuccess) {
            delete hp;
            if (c->d_params185) { (void)hipFree(c->d_params185); c->d_params185 = nullptr; }
            return fail(c, -6, "mirp_set_fold_model: device allocation failed");
        }
        delete hp;
    }
    c->fold_model = model;
    c->have_fold = false; c->have_result = false;
    return 0;
}

extern "C" void mirp_destroy(mirp_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)mirp_wait_text(c);
    (void)mirp_dist_finalize(c);
    for (int i = 0; i < 6; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (hipEvent_t ev : c->fold_ev) (void)hipEventDestroy(ev);
    if (c->stream_epi) (void)hipStreamDestroy(c->stream_epi);
    if (c->stream_fill2) (void)hipStreamDestroy(c->stream_fill2);
    if (c->d_params) (void)hipFree(c->d_params);
    if (c->d_params185) (void)hipFree(c->d_params185);
    if (c->d_params185l) (void)hipFree(c->d_params185l);
    if (c->stream) { mirp::release_scan_scratch(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;      // ~DevBuf frees every device buffer of the context, behind its streams and events
}

extern "C" const char* mirp_last_error(const mirp_ctx* c) { return c ? c->err.c_str() : "null context"; }
extern "C" void mirp_free(void* p) { std::free(p); }

static int fold_batch_impl(mirp_ctx* c, const char* seqs, const int64_t* offsets, int32_t n_seqs, int32_t span,
                           int32_t max_lines, MirpFoldLine** lines, char** ss, int32_t* ss_stride_out,
                           int32_t** n_lines, int32_t** mfe, int32_t** status, bool want_text) {
    if (!c) return -1;
    if (!seqs || !offsets || n_seqs < 0 || (want_text && (!lines || !ss || !ss_stride_out)) || !n_lines || !mfe || !status)
        return fail(c, -1, "mirp_fold_batch: null argument");
    int32_t stride_dummy = 0;
    if (!ss_stride_out) ss_stride_out = &stride_dummy;
    if (span < 1 || max_lines < 1) return fail(c, -1, "mirp_fold_batch: bad span/max_lines");
    HIPCHK(c, hipSetDevice(c->device));
    int n_max = 1;
    for (int i = 0; i < n_seqs; i++) {
        int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0) return fail(c, -1, "mirp_fold_batch: offsets not monotone");
        if (n > MIRP_NMAX) return fail(c, -5, "mirp_fold_batch: sequence longer than MIRP_NMAX");
        n_max = std::max<int>(n_max, (int)n);
    }
    const int stride = ((n_max + 3 + 7) / 8) * 8;
    *ss_stride_out = stride;
    const size_t nl = (size_t)n_seqs * max_lines;
    MirpFoldLine* h_lines = (MirpFoldLine*)std::calloc(want_text ? std::max<size_t>(nl, 1) : 1, sizeof(MirpFoldLine));
    char* h_ss = (char*)std::calloc(want_text ? std::max<size_t>(nl * stride, 1) : 1, 1);
    int32_t* h_nl = (int32_t*)std::calloc(std::max(n_seqs, 1), sizeof(int32_t));
    int32_t* h_mfe = (int32_t*)std::calloc(std::max(n_seqs, 1), sizeof(int32_t));
    int32_t* h_st = (int32_t*)std::calloc(std::max(n_seqs, 1), sizeof(int32_t));
    auto bail = [&](int code, const std::string& m) {
        std::free(h_lines); std::free(h_ss); std::free(h_nl); std::free(h_mfe); std::free(h_st);
        return fail(c, code, m);
    };
    if (!h_lines || !h_ss || !h_nl || !h_mfe || !h_st) return bail(-6, "mirp_fold_batch: host allocation failed");
    if (n_seqs > 0) {
        const size_t total = (size_t)offsets[n_seqs] - (size_t)offsets[0];
        if (c->seqs.ensure(total + 16) || c->offs.ensure(sizeof(long long) * (n_seqs + 1)))
            return bail(-6, "device allocation failed (inputs)");
        std::vector<long long> rel(n_seqs + 1);
        for (int i = 0; i <= n_seqs; i++) rel[i] = offsets[i] - offsets[0];
        if (hipMemcpyAsync(c->seqs.p, seqs + offsets[0], total, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->offs.p, rel.data(), sizeof(long long) * (n_seqs + 1), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return bail(-2, "H2D copy failed");
        // batches bound the structure-text buffer
        const size_t per_win = (size_t)max_lines * stride;
        int batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_seqs, ((size_t)1 << 30) / per_win));
        // the batch path has its own output buffers: a batch call between mirp_fold and mirp_predict (the imported windows of a re-balanced run,
        // balance.py) must not touch the resident fold output
        if (c->blines.ensure(sizeof(MirpFoldLine) * (size_t)batch * max_lines) || c->bss.ensure((size_t)batch * per_win) ||
            c->bnlines.ensure(4 * (size_t)n_seqs) || c->bmfe.ensure(4 * (size_t)n_seqs) || c->bstatus.ensure(4 * (size_t)n_seqs))
            return bail(-6, "device allocation failed (outputs)");
        double kms[2] = {0, 0};
        long long fallbacks = 0;
        for (int b0 = 0; b0 < n_seqs; b0 += batch) {
            const int nb = std::min(batch, n_seqs - b0);
            // windows of this batch are addressed relative to b0: shift the pointers
            int rc = mirp_run_fold(c, (const unsigned char*)c->seqs.p, (const long long*)c->offs.p + b0, nullptr, nb, n_max, span, max_lines, stride,
                                   (MirpFoldLine*)c->blines.p, (char*)c->bss.p, (int*)c->bnlines.p + b0, (int*)c->bmfe.p + b0, (int*)c->bstatus.p + b0);
            if (rc) return bail(rc, c->err);
            kms[0] += c->fold_kernel_ms[0]; kms[1] += c->fold_kernel_ms[1]; fallbacks += c->last_fallback;
            if (want_text &&
                (hipMemcpyAsync(h_lines + (size_t)b0 * max_lines, c->blines.p, sizeof(MirpFoldLine) * (size_t)nb * max_lines,
                                hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                 hipMemcpyAsync(h_ss + (size_t)b0 * per_win, c->bss.p, (size_t)nb * per_win, hipMemcpyDeviceToHost, c->stream) != hipSuccess))
                return bail(-2, "D2H copy failed");
            if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(-2, "fold kernel execution failed");
        }
        c->fold_kernel_ms[0] = kms[0]; c->fold_kernel_ms[1] = kms[1]; c->last_fallback = fallbacks;      // over all batches of this call
        if (hipMemcpy(h_nl, c->bnlines.p, 4 * (size_t)n_seqs, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h_mfe, c->bmfe.p, 4 * (size_t)n_seqs, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h_st, c->bstatus.p, 4 * (size_t)n_seqs, hipMemcpyDeviceToHost) != hipSuccess)
            return bail(-2, "D2H copy failed");
    }
    if (want_text) { *lines = h_lines; *ss = h_ss; } else { std::free(h_lines); std::free(h_ss); }
    *n_lines = h_nl; *mfe = h_mfe; *status = h_st;
    return 0;
}

extern "C" int mirp_fold_batch(mirp_ctx* c, const char* seqs, const int64_t* offsets, int32_t n_seqs, int32_t span,
                               int32_t max_lines, MirpFoldLine** lines, char** ss, int32_t* ss_stride_out,
                               int32_t** n_lines, int32_t** mfe, int32_t** status) {
    return fold_batch_impl(c, seqs, offsets, n_seqs, span, max_lines, lines, ss, ss_stride_out, n_lines, mfe, status, true);
}

extern "C" int mirp_fold_batch_summary(mirp_ctx* c, const char* seqs, const int64_t* offsets, int32_t n_seqs, int32_t span, int32_t max_lines,
                                       int32_t** n_lines, int32_t** mfe, int32_t** status) {
    return fold_batch_impl(c, seqs, offsets, n_seqs, span, max_lines, nullptr, nullptr, nullptr, n_lines, mfe, status, false);
}

// ------------------------------------------------------------------------------------------
template <class T>
static T* host_alloc(size_t n) { return (T*)std::calloc(std::max<size_t>(n, 1), sizeof(T)); }

static int predict_batch_impl(mirp_ctx* c, const MirpWindow* windows, int32_t n_windows, const MirpMature* matures, int64_t n_matures,
                              const MirpAln* alns, int64_t n_alns, const MirpFoldLine* lines, const char* ss, int32_t ss_stride,
                              int32_t max_lines, const int32_t* n_lines, const MirpPredictParams* pp, MirpMirna** mirnas,
                              int32_t** n_mirnas, int32_t** status, int32_t** reasons, int64_t* n_reasons, int32_t* reasons_stride) {
    if (!c) return -1;
    if (!windows || !matures || !alns || !lines || !ss || !n_lines || !pp || !mirnas || !n_mirnas || !status || n_windows < 0)
        return fail(c, -1, "mirp_predict_batch: null argument");
    if (pp->n_samples < 1 || pp->n_samples > MIRP_MAX_SAMPLES) return fail(c, -1, "mirp_predict_batch: n_samples out of range");
    if (ss_stride % 8 != 0) return fail(c, -1, "mirp_predict_batch: ss_stride must be a multiple of 8");
    HIPCHK(c, hipSetDevice(c->device));
    if (mirp::predict_lds_bytes_min(max_lines, ss_stride) > 160 * 1024)
        return fail(c, -5, "mirp_predict_batch: max_lines*ss_stride exceeds the LDS budget of the predict kernel");
    TmpDevice T;
    const size_t nl = (size_t)n_windows * max_lines;
    void* d_w = T.get(sizeof(MirpWindow) * n_windows);
    void* d_m = T.get(sizeof(MirpMature) * n_matures);
    void* d_a = T.get(sizeof(MirpAln) * n_alns);
    void* d_l = T.get(sizeof(MirpFoldLine) * nl);
    void* d_s = T.get(nl * ss_stride);
    void* d_n = T.get(4 * (size_t)n_windows);
    void* d_o = T.get(sizeof(MirpMirna) * (size_t)n_windows * MIRP_MAX_MIRNA_PER_WINDOW);
    void* d_no = T.get(4 * (size_t)n_windows);
    void* d_st = T.get(4 * (size_t)n_windows);
    if (!d_w || !d_m || !d_a || !d_l || !d_s || !d_n || !d_o || !d_no || !d_st) return fail(c, -6, "device allocation failed");
    MirpMirna* h_o = host_alloc<MirpMirna>((size_t)n_windows * MIRP_MAX_MIRNA_PER_WINDOW);
    int32_t* h_no = host_alloc<int32_t>(n_windows);
    int32_t* h_st = host_alloc<int32_t>(n_windows);
    auto bail = [&](int code, const std::string& m) { std::free(h_o); std::free(h_no); std::free(h_st); return fail(c, code, m); };
    if (n_windows > 0) {
        if (hipMemcpyAsync(d_w, windows, sizeof(MirpWindow) * n_windows, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_m, matures, sizeof(MirpMature) * n_matures, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_a, alns, sizeof(MirpAln) * n_alns, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_l, lines, sizeof(MirpFoldLine) * nl, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_s, ss, nl * ss_stride, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(d_n, n_lines, 4 * (size_t)n_windows, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return bail(-2, "H2D copy failed");
        int grid = std::min(n_windows, c->n_cu * 16);
        // reasons mode (-d): one int32 record per window and per evaluated (mature, structure) pair, layout as mirp_predict_reasons
        const int rstride = 21 + pp->n_samples;
        unsigned int rcap = reasons ? (unsigned int)std::min<unsigned long long>((unsigned long long)n_windows * 96ull + 1024ull, 0x7fffffffull / (unsigned)rstride) : 0u;
        unsigned int* d_cnt = reasons ? (unsigned int*)T.get(16) : nullptr;
        int* d_pool = reasons ? (int*)T.get((size_t)rcap * rstride * 4) : nullptr;
        if (reasons && (!d_cnt || !d_pool)) return bail(-6, "device allocation failed (reasons pool)");
        if (reasons && hipMemsetAsync(d_cnt, 0, 16, c->stream) != hipSuccess) return bail(-2, "memset failed");
        (void)grid;
        {
            std::string err;
            c->reset_jobs_per_slot(4);
            if (int rc = mirp::run_predict_launch(c->stream, c->n_cu, (const MirpWindow*)d_w, n_windows, (const MirpMature*)d_m, (const MirpAln*)d_a, n_alns,
                                                  (const MirpFoldLine*)d_l, (const char*)d_s, ss_stride, max_lines, (const int*)d_n, *pp, (MirpMirna*)d_o,
                                                  (int*)d_no, (int*)d_st, d_cnt, d_pool, rcap, rstride, nullptr, 0, nullptr, &err, nullptr, c->jobs_per_slot[4]))
                return bail(rc, "mirp_predict_batch: " + err);
        }
        if (reasons) {
            unsigned int n = 0;
            if (hipMemcpyAsync(&n, d_cnt, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
                return bail(-2, "predict kernel execution failed");
            if (n > rcap) return bail(-6, "mirp_predict_batch_reasons: record pool overflow");
            int32_t* h = host_alloc<int32_t>((size_t)n * rstride);
            if (!h || (n && hipMemcpy(h, d_pool, (size_t)n * rstride * 4, hipMemcpyDeviceToHost) != hipSuccess)) { std::free(h); return bail(-2, "D2H copy failed"); }
            size_t k2 = 0;          // records of a first pass whose window was run again at larger capacities carry window -1
            for (size_t k = 0; k < n; k++)
                if (h[k * rstride] >= 0) { if (k2 != k) std::memcpy(h + k2 * rstride, h + k * rstride, 4 * (size_t)rstride); k2++; }
            *reasons = h; *n_reasons = (int64_t)k2; *reasons_stride = rstride;
        }
        if (hipMemcpyAsync(h_o, d_o, sizeof(MirpMirna) * (size_t)n_windows * MIRP_MAX_MIRNA_PER_WINDOW, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(h_no, d_no, 4 * (size_t)n_windows, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(h_st, d_st, 4 * (size_t)n_windows, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return bail(-2, "predict kernel execution failed");
    }
    *mirnas = h_o; *n_mirnas = h_no; *status = h_st;
    return 0;
}

extern "C" int mirp_predict_batch(mirp_ctx* c, const MirpWindow* windows, int32_t n_windows, const MirpMature* matures, int64_t n_matures,
                                  const MirpAln* alns, int64_t n_alns, const MirpFoldLine* lines, const char* ss, int32_t ss_stride,
                                  int32_t max_lines, const int32_t* n_lines, const MirpPredictParams* pp, MirpMirna** mirnas,
                                  int32_t** n_mirnas, int32_t** status) {
    return predict_batch_impl(c, windows, n_windows, matures, n_matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, mirnas, n_mirnas, status,
                              nullptr, nullptr, nullptr);
}

extern "C" int mirp_predict_batch_reasons(mirp_ctx* c, const MirpWindow* windows, int32_t n_windows, const MirpMature* matures, int64_t n_matures,
                                          const MirpAln* alns, int64_t n_alns, const MirpFoldLine* lines, const char* ss, int32_t ss_stride,
                                          int32_t max_lines, const int32_t* n_lines, const MirpPredictParams* pp, MirpMirna** mirnas,
                                          int32_t** n_mirnas, int32_t** status, int32_t** reasons, int64_t* n_reasons, int32_t* reasons_stride) {
    if (!reasons || !n_reasons || !reasons_stride) return fail(c, -1, "mirp_predict_batch_reasons: null argument");
    *reasons = nullptr; *n_reasons = 0; *reasons_stride = 0;
    return predict_batch_impl(c, windows, n_windows, matures, n_matures, alns, n_alns, lines, ss, ss_stride, max_lines, n_lines, pp, mirnas, n_mirnas, status,
                              reasons, n_reasons, reasons_stride);
}

// Read collapse of scripts/process-reads-fasta.py:60-80 for one file (reads_kernels.hip does the device part).
extern "C" int mirp_collapse_reads(mirp_ctx* c, const char* path, const char* prefix, const char* out_path, int32_t hash_bits, int64_t* n_reads,
                                   int64_t* n_unique, double seconds[6]) {
    if (!c) return -1;
    if (!path || !prefix || !out_path || hash_bits < 1 || hash_bits > 64) return fail(c, -1, "mirp_collapse_reads: bad argument");
    double sec[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(c, hipSetDevice(c->device));
    double t = mirp::now();
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(c, -8, std::string("cannot open ") + path);
    fseeko(f, 0, SEEK_END);
    const long long n = (long long)ftello(f);
    fseeko(f, 0, SEEK_SET);
    char* text = (char*)std::malloc((size_t)n + 1);
    if (!text) { std::fclose(f); return fail(c, -7, "host allocation failed (collapse: text)"); }
    const size_t got = n > 0 ? std::fread(text, 1, (size_t)n, f) : 0;
    std::fclose(f);
    if ((long long)got != n) { std::free(text); return fail(c, -8, std::string("cannot read ") + path); }
    sec[0] = mirp::now() - t;
    char* out = nullptr;
    long long out_len = 0, nr = 0, nu = 0, bad = -1;
    const int rc = mirp_device_collapse_reads(c, text, n, prefix, hash_bits, &out, &out_len, &nr, &nu, &bad, sec);
    if (rc == -9) {
        char msg[160];
        std::snprintf(msg, sizeof msg, ": byte 0x%02x at offset %lld is not ASCII (bytes >= 0x80 are not supported)", (unsigned)(unsigned char)text[bad], bad);
        c->err = std::string(path) + msg;
    }
    std::free(text);
    if (rc) return rc;
    t = mirp::now();
    mirp::OutFile o(out_path);
    const bool ok = o.write(out, (size_t)out_len) && o.commit();
    std::free(out);
    if (!ok) return fail(c, -8, std::string("cannot write ") + out_path);
    sec[5] = mirp::now() - t;
    if (n_reads) *n_reads = nr;
    if (n_unique) *n_unique = nu;
    if (seconds) std::memcpy(seconds, sec, sizeof sec);
    return 0;
}

extern "C" int64_t mirp_last_collapse_collisions(const mirp_ctx* c) { return c ? c->last_collapse_collisions : -1; }

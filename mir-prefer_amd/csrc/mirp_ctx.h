// Context and helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "mirp_internal.h"

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;              // owns its allocation: never copied, freed when its owner goes (~mirp_ctx frees every buffer of a context)
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
};

struct TmpDevice {   // scoped device allocations
    std::vector<void*> ptrs;
    ~TmpDevice() { for (void* p : ptrs) (void)hipFree(p); }
    void* get(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
};

struct mirp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int n_cu = 256;
    FoldParams* d_params = nullptr;
    FoldParams185* d_params185 = nullptr;   // created on the first use of the vienna-1.8.5 model (generic kernel)
    FoldParams* d_params185l = nullptr;     // Turner-1999 values in the layout of the LDS-resident kernels
    int fold_model = MIRP_FOLD_MODEL_VIENNA_212;
    DevBuf seqs, offs, ws, lines, ss, nlines, mfe, status, carch, fctl, flist, wstate, dlist;
    DevBuf blines, bss, bnlines, bmfe, bstatus;      // outputs of mirp_fold_batch (kept apart from the resident fold output of mirp_fold)
    long long last_fallback = 0;
    // ---- device-resident pipeline state (mirp_pipeline.cpp)
    int n_contigs = 0;
    long long gtot = 0, gbytes = 0, n_alns = 0;
    std::vector<long long> h_clen, h_goff, h_gboff;
    DevBuf genome, clen, goff, gboff, alns, order, segs, sort_tmp, sort_counts;
    long long n_segs = 0;
    DevBuf tile_first;               // fused coverage scan: first record of every tile (candidate_kernels.hip)
    int max_aln_len = -1;             // longest resident record (reference span), -1 = not known: the fused scan needs it <= one tile
    int fold_dense = 0;               // mirp_set_fold_split_path: 1 = dense multiloop splits for every window
    unsigned int last_dense = 0;      // windows of the last fold the candidate-pool pass handed to the dense fill kernel
    int cov_mode = -1;                // mirp_set_coverage_path: -1 = by record density, 0 = atomic scatter, 1 = fused scan (where the input allows it)
    bool cov_fused = false;           // the last run_coverage took the fused path (nothing to clear afterwards)
    void* diff_clean_ptr = nullptr;   // the difference arrays at this address are all zero (run_coverage / clean_coverage)
    size_t diff_clean_bytes = 0;
    bool ingest_resident = false;     // the alignments came from mirp_ingest_sams_gpu (already validated and sorted on the device)
    int ingest_n_contigs = 0;
    DevBuf diff, stat, starts, totals, runs, keep, kscan, csq, cdest, peaks_sq, peaks_sorted;
    DevBuf head, hscan, rfirst, nent, isloc, nslots, escan, lscan, sscan, windows, roles, loci, wpeaks, matures, wseqs, woffs, wlens;
    DevBuf p_out, p_nout, p_status, p_keep, p_kscan, p_res, p_text, p_need;
    // windows whose structure lines exceed the default capacity: re-folded alone at full capacity into these side buffers (mirp_fold)
    DevBuf side_cnt, side_idx, side_list, side_offs, side_lens, lines2, ss2, nlines2, mfe2, status2;
    long long n_side = 0;
    int side_max_lines = 0;
    MirpCandidateParams cand = {0, 0, 0, 0};
    long long n_runs = 0, n_above = 0, n_peaks = 0, n_regions = 0, n_loci = 0, n_windows = 0, n_slots = 0;
    int seq_stride = 0, fold_stride = 0, fold_max_lines = 0, fold_span = 0;
    bool have_candidate = false, have_fold = false;
    int shard_first_run_double = 0;   // contig shard whose first covered contig is not the first covered contig of the whole genome
    double ms[4] = {0, 0, 0, 0};
    double fold_kernel_ms[2] = {0, 0};   // fill / epilogue kernels of the last mirp_run_fold (LDS-resident path)
    std::vector<hipEvent_t> fold_ev;     // the fold's events, created on demand; mirp_fold.cpp names the ones a path uses
    int fold_prepared_lines = -1;        // max_lines that fold_lds_prepare and overlap_epi_wgs were last asked at on this context's device, -1 = not yet
    // ---- fold overlap (mirp_run_fold): the epilogue of a chunk of windows runs on a stream of its own beside the fill of the next chunk
    int fold_overlap = -1;               // mirp_set_fold_overlap: -1 = automatic, 0 = off (serial path), N > 0 = chunks of N windows
    int overlap_epi_wgs = -1;            // epilogue workgroups a CU holds beside two fill workgroups (fold_lds_overlap_epi_wgs) at fold_prepared_lines structure lines
    int fold_tailfree = -1;              // mirp_set_fold_overlap_tailfree: -1 = automatic (on), 0 = fills in order on one stream and a dense pass per chunk, 1 = on
    hipStream_t stream_epi = nullptr;    // created on the first chunked fold
    hipStream_t stream_fill2 = nullptr;  // the fills of the odd chunks (tail-free schedule); created on the first fold that needs it
    int last_overlap_chunks = 0;         // chunks of the last mirp_run_fold (0: serial path)
    long long fold_cap = 0;              // windows whose slabs are resident at once; 0 = the default, 8 GiB of slabs (mirp_set_fold_capacity)
    // ---- fold dedup (mirp_fold, fold_dedup_kernels.hip): a window that repeats an earlier one byte for byte is not folded, it gets that window's results
    int fold_dedup = 1;                  // mirp_set_fold_dedup: 0 = every window is folded
    int fold_dedup_bits = 0;             // mirp_set_fold_dedup_hash_bits: bits of the hash that count, 0 = all 64 (lowered only to test collisions)
    DevBuf dd;                           // FoldDedupLayout of the last mirp_fold
    long long dd_windows = -1;           // windows of the map in `dd`, -1 = the last mirp_fold looked for no duplicates
    long long last_duplicates = 0;       // duplicates the last mirp_fold skipped
    // what mirp_fold hands mirp_run_fold for one call (other callers leave n_dup null: nothing is counted, nothing more is launched), and what it
    // gets back: the duplicates of the windows that went to the generic kernel / the dense passes, and the call's duplicates (-1: no read-back took them)
    struct FoldDupRun { const int* n_dup = nullptr; const unsigned* total = nullptr; long long fallbacks = 0, dense = 0, duplicates = -1; } dup_run;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // ---- multi-GPU (mirp_dist.cpp): RCCL communicator of this context's device, one process per GPU
    void* comm = nullptr;
    int dist_rank = 0, dist_world = 1;
    std::string dist_dir;             // local transport (mirp_dist_init_local): ranks that share a GPU exchange through files in this directory
    long long dist_seq = 0;
    bool dist_broken = false;         // a wait on a peer expired (or RCCL reported an asynchronous error): the communicator was aborted, every later exchange fails at once
    DevBuf dist_tmp;
    struct TextJob { std::thread th; int rc = 0; std::string err; };
    std::vector<std::shared_ptr<TextJob>> text_jobs;      // text artefacts still being formatted / written behind the caller (mirp_wait_text)
    // window view (mirp_select_windows): the fold and the filter run on windows [win_first, win_first + n_windows) of the candidate stage's list;
    // sel_total = the list's length while a view is active, -1 otherwise
    long long win_first = 0, sel_total = -1;
    const MirpWindow* v_windows() const { return (const MirpWindow*)windows.p + win_first; }
    const int* v_roles() const { return (const int*)roles.p + win_first; }
    const long long* v_woffs() const { return (const long long*)woffs.p + win_first; }
    const int* v_wlens() const { return (const int*)wlens.p + win_first; }
    // ---- read collapse (reads_kernels.hip): the file text and the per-line / per-read arrays, reused from file to file
    DevBuf r_text, r_bcnt, r_bscan, r_starts, r_flag, r_fscan, r_span, r_rec, r_rectmp, r_rscan, r_first, r_bad, r_cnt, r_isfirst, r_inbad, r_rank, r_out, r_small;
    long long last_collapse_collisions = 0;   // reads in hash runs that failed the byte compare (resolved on the host)
    // ---- read alignment (align_kernels.hip, mirp_align.cpp): the packed reference and its index stay resident between mirp_align_reads calls
    DevBuf a_pk, a_amb, a_cst, a_cstart, a_names, a_noff, a_sa, a_bkt;
    long long a_total = 0, a_nsa = 0;
    int a_n_contigs = 0;
    bool a_ready = false;
    long long a_batches = 0;          // batches of the last mirp_align_reads (mirp_align_last_batches)
    std::vector<std::string> a_contig_names;
    std::vector<long long> a_contig_lens;
    DevBuf a_codes, a_roff, a_qn, a_qoff, a_small, a_rcnt, a_rscan, a_seeds, a_ccnt, a_cscan, a_lvl, a_best, a_supp, a_slots, a_off, a_cursor, a_items, a_itmp,
        a_size, a_toff, a_text;
    // placement (mirp_align_reads_placed): the reads' depths, the unique list of the file (gpos << 32 | depth), its sorted positions and depth
    // prefix, the weights of a batch's items and the per-read picks and tag fields
    DevBuf a_depth, a_ulist, a_utmp, a_upos, a_ulo, a_uhi, a_uls, a_uhs, a_upre, a_w, a_pick, a_pn, a_pcls, a_pw, a_pwt;
    // tails (mirp_align_reads_tailed, align_tail_kernels.hip): the batch's reads without a hit, their seeds' SA ranges and candidate scan, the hit
    // counts per tail length, the per-read tail length, and the file's summary table ((reads, depth) per tail string, resident over its batches)
    DevBuf a_tlist, a_tslo, a_tccnt, a_tcscan, a_tlvl, a_tt, a_thist;
    long long a_tail_nq = 0, a_tail_tc = 0;   // searched reads and candidates of the batch whose hits are being made
    long long a_place_cap = 0;        // items of pass 1 kept resident for pass 2; 0 = the default, 2^28 (mirp_set_align_place_capacity)
    long long a_place_realigned = 0;  // batches the last mirp_align_reads_placed aligned twice (mirp_align_place_last_realigned)
    std::vector<char> h_text;        // one piece (<= text_piece_bytes()) of the SAM text on its way to the file
    long long text_piece = 0;        // bytes of text per piece; 0 = the default, 1 GiB (mirp_set_text_piece: lowered only to test the piece path)
    long long text_pieces = 0;       // non-empty pieces handed to a sink since the last call that emits text started (mirp_text_pieces_last)
    long long text_piece_bytes() const { return text_piece > 0 ? text_piece : 1ll << 30; }
    // ---- read trimming (trim_kernels.hip, mirp_trim.cpp): the file text, its lines and the per-read arrays, reused from file to file
    DevBuf t_text, t_bcnt, t_bscan, t_starts, t_small, t_hdr, t_llen, t_lb, t_hscan, t_goff, t_first, t_gbuf, t_src, t_len, t_qual, t_nameb, t_namel,
        t_flen, t_off, t_out;
    long long t_paths[2] = {0, 0};    // workgroups of the last mirp_trim_reads that staged their reads in LDS / read them from global memory (mirp_trim_last_paths)
    // ---- library profile (libqc_kernels.hip, mirp_libqc.cpp): the 4^12 k-mer counters, the found adapter with the walk's scratch, the three tables;
    // the text, lines and per-read arrays are the trim's (t_*)
    DevBuf q_table, q_found, q_hist;
    bool q_have_table = false;        // q_table holds the counters of the last mirp_libqc_reads (mirp_libqc_last_table); false after a refused call
    // ---- target-site search (targets_kernels.hip, mirp_targets.cpp): the packed targets, the miRNAs and the key / text buffers of one call
    DevBuf tg_pk, tg_amb, tg_cst, tg_cstart, tg_names, tg_noff, tg_mcodes, tg_mnames, tg_mnoff, tg_mi, tg_emitted, tg_hist, tg_small, tg_keys, tg_ktmp,
        tg_size, tg_toff, tg_text;
    long long tg_cap = 0;             // keys held per pass; 0 = the default, 2^26 (mirp_set_target_capacity)
    // ---- known-miRNA annotation (annotate_kernels.hip, mirp_annotate.cpp): the packed and the planar sequences, the hits per query and the cut
    // tables of one pass; the keys use tg_keys / tg_ktmp / tg_small / tg_hist
    DevBuf an_pack, an_q, an_k, an_cnt, an_run, an_out, an_kept;
    // ---- shuffle test of precursor MFEs (randfold_kernels.hip, mirp_randfold.cpp): the sequences of the call (codes, offsets, order, cumulated lengths,
    // records) and the buffers of one pass: the shuffled sequences and their offsets as the fold reads them, the successor lists, the fold's outputs
    DevBuf rf_codes, rf_offs, rf_perm, rf_cum, rf_rec, rf_bad, rf_seq, rf_soffs, rf_slab, rf_lines, rf_ss, rf_nlines, rf_mfe, rf_status;
    // ---- two-strand fold (duplex_kernels.hip, mirp_duplex.cpp): the coded strands and offsets of one pass of mirp_duplex_batch and its results;
    // with targets -e the results per key of a pass (tg_e*) and the perfect duplex per miRNA of a group (tg_perf)
    DevBuf dx_a, dx_b, dx_aoff, dx_boff, dx_mfe, dx_ma, dx_mb, dx_small, tg_emfe, tg_ema, tg_emb, tg_perf;
    long long dx_cap = 0;             // pairs per pass of mirp_duplex_batch; 0 = the default, 2^20 (mirp_set_duplex_capacity)
    long long dx_stats[3] = {0, 0, 0};   // the last mirp_duplex_batch: pairs, passes, loop evaluations
    // ---- partition function (ensemble_kernels.hip, mirp_ensemble.cpp): the letters and codes of the call, the MFE fold's outputs, the jobs, slabs,
    // records, texts and pair lists of one pass
    DevBuf en_seq, en_soffs, en_codes, en_lines, en_ss, en_nlines, en_mfe, en_status, en_jobs, en_slab, en_recs, en_texts, en_rowcnt, en_rowat, en_bpp;
    long long en_cap = 0;             // slab bytes per pass of mirp_ensemble; 0 = the default, 2^35 (mirp_set_ensemble_capacity)
    long long en_stats[3] = {0, 0, 0};   // the last mirp_ensemble: sequences, passes, cells
    // ---- accessibility of intervals (unpaired_kernels.hip, mirp_unpaired.cpp): the coded windows, offsets, intervals, binned order and records of
    // one pass, and the wave-private slabs of the windows too long for LDS; with targets -u the records per key of a pass (tg_upe)
    DevBuf up_codes, up_offs, up_lo, up_hi, up_order, up_recs, up_slab, tg_upe;
    long long up_cap = 0;             // windows per pass of mirp_unpaired_batch; 0 = the default, 2^20 (mirp_set_unpaired_capacity)
    long long up_stats[3] = {0, 0, 0};   // the last mirp_unpaired_batch: windows, passes, cells
    int tg_up = 17, tg_down = 13;     // the flanks of targets -u (mirp_set_target_flanks)
    // ---- gapped alignment with known hairpins (hairpin_kernels.hip, mirp_hairpin.cpp): the coded queries and known sequences of the call, the
    // known sequences packed per wave, the boundary rows between strips, the results, keys and cut tables of one scoring pass, the hits, direction
    // matrices and ops of one traceback pass
    DevBuf hp_q, hp_qat, hp_qlen, hp_k, hp_kat, hp_kw, hp_waves, hp_korig, hp_carry, hp_res, hp_cnt, hp_small, hp_keys, hp_ktmp, hp_run, hp_out, hp_kept,
        hp_hits, hp_jobs, hp_dir, hp_ops;
    long long hp_cap = 0;             // bytes per pass of mirp_hairpin_align; 0 = the default, 2^31 (mirp_set_hairpin_capacity)
    long long hp_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the last mirp_hairpin_align: queries, known, pairs, cells, hits, passes, scoring passes, traceback passes
    double hp_sec[5] = {0, 0, 0, 0, 0};                 // upload, scoring, filter + sort + cut, traceback, download
    std::vector<long long> hp_per_query;                // hits of every query of the last call, before the cut
    // ---- homolog search (homolog_kernels.hip, mirp_homolog.cpp): the queries and keys use the read alignment's buffers (a_*); the keys, windows,
    // letters, offsets, evaluation records, winning texts, needs and re-run list of one chunk of placements; the fold's output goes to b*
    DevBuf hm_keys, hm_win, hm_lens, hm_offs, hm_seqs, hm_eval, hm_ss, hm_need, hm_sel;
    long long hm_cap = 0, hm_chunk = 0;   // keys per scan pass (0 = 2^24) and windows per fold chunk (0 = by the fold output's size) (mirp_set_homolog_capacity)
    int hm_lines = 0;                     // structure lines the fold keeps per window at first (0 = 96)
    int hm_eval_caps[3] = {0, 0, 0};      // pieces per line, structures and staged lines of the evaluation's first launch (0 = the defaults)
    long long hm_stats[24] = {0};         // the last mirp_homolog_scan (mirp_homolog_last_stats)
    double hm_sec[5] = {0, 0, 0, 0, 0};
    // ---- target-mimic search (mimic_kernels.hip, mirp_mimics.cpp): the seed start table, the file index of every miRNA in seed order and the
    // lengths in file order; the packed targets, names, miRNA masks, keys and text use the target-site search's buffers (tg_*)
    DevBuf mm_start, mm_mid, mm_len;
    // ---- inverted repeats (inverted_kernels.hip, mirp_inverted.cpp): the packed contigs and their padded starts and ends, the row keys, the
    // candidate keys and the jobs, records, direction bytes and ops of one traceback pass
    DevBuf iv_words, iv_pstart, iv_pend, iv_keys, iv_cand, iv_ctmp, iv_small, iv_jobs, iv_recs, iv_dir, iv_ops;
    long long iv_cap = 0;             // bytes per pass of mirp_inverted_scan; 0 = the default, 2^31 (mirp_set_inverted_capacity)
    long long iv_stats[12] = {0};     // the last mirp_inverted_scan (mirp_inverted_last_stats)
    double iv_sec[5] = {0, 0, 0, 0, 0};
    // ---- natural antisense transcripts (nats_kernels.hip, mirp_nats.cpp): the transcripts and their reverse complements as 4-bit codes, the
    // transcript of every word and the first nibble of every transcript; the k-mer records and their sort buffer, the run heads, their scan and
    // the runs' starts, the hits per transcript a; the hit keys of one join pass, its candidates; the jobs and results of the band scan; the
    // jobs, records, direction bytes and ops of one traceback pass
    DevBuf nt_a, nt_b, nt_wseq, nt_pos, nt_recs, nt_rtmp, nt_flag, nt_scan, nt_starts, nt_cnt, nt_small, nt_hits, nt_htmp, nt_cand, nt_jobs, nt_best, nt_tjobs,
        nt_trec, nt_dir, nt_ops;
    long long nt_cap = 0;             // bytes per pass of mirp_nats_scan; 0 = the default, 2^31 (mirp_set_nats_capacity)
    long long nt_stats[16] = {0};     // the last mirp_nats_scan (mirp_nats_last_stats)
    double nt_sec[6] = {0, 0, 0, 0, 0, 0};
    long long n_result = 0;          // records of the last mirp_predict (p_res / p_text), what mirp_gather_loci sends
    bool have_result = false;
    // ---- jobs per resident slot (mirp_last_jobs_per_slot): per family (0 duplex_kernel, 1 unpaired_kernel, 2 hp_score_kernel, 3 homolog_eval_kernel, 4 predict_kernel, 5 lc_count_kernel, 6 de_sum_kernel, 7 sg_overlap_kernel, 8 nt_scan_kernel)
    // the launches of the last C-ABI call that can launch it and the largest ceil(jobs / slots) among them; a record, read by nothing in the library
    long long jobs_per_slot[9][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
    void reset_jobs_per_slot(int family) { jobs_per_slot[family][0] = jobs_per_slot[family][1] = 0; }
    void note_jobs_per_slot(int family, long long jobs, long long slots) {
        jobs_per_slot[family][0]++;
        jobs_per_slot[family][1] = std::max(jobs_per_slot[family][1], (jobs + slots - 1) / slots);          // every launch has slots >= 1
    }
};

static inline int fail(mirp_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail((c), -2, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace mirp {
// seconds on the steady clock: what every `seconds[]` of the C ABI is measured with
inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace mirp

// Copies `bytes` of device text to the host through c->h_text in pieces of at most c->text_piece_bytes() (1 GiB unless a test lowered it) and hands
// every piece to the sink, counting it in c->text_pieces; the seconds spent inside the sink are added to *in_sink when it is given.
inline int mirp_download_text(mirp_ctx* c, const char* d_text, long long bytes, const std::function<int(const char*, size_t)>& sink, double* in_sink = nullptr) {
    const size_t piece = (size_t)c->text_piece_bytes();
    if (bytes > 0 && c->h_text.size() < std::min((size_t)bytes, piece)) c->h_text.resize(std::min((size_t)bytes, piece));
    for (long long at = 0; at < bytes;) {
        const size_t len = (size_t)std::min<long long>(bytes - at, (long long)piece);
        HIPCHK(c, hipMemcpy(c->h_text.data(), d_text + at, len, hipMemcpyDeviceToHost));
        const double t = mirp::now();
        c->text_pieces++;
        if (int rc = sink(c->h_text.data(), len)) return rc;
        if (in_sink) *in_sink += mirp::now() - t;
        at += (long long)len;
    }
    return 0;
}

// sort_kernels.hip: stable device sort by (tid, pos) / keep-region filter of the resident record array.  Every sort orders by whole 8-bit digits, the
// key bits [base, base + 8 * ceil(bits / 8)): callers keep the bits above their `bits` equal or meaningful.
int mirp_device_sort_alns(mirp_ctx* c, MirpAln* d_alns, MirpAln* d_tmp, long long n, int posbits, int tidbits);
int mirp_device_sort_u64(mirp_ctx* c, unsigned long long* d, unsigned long long* d_tmp, long long n, int base, int bits);
int mirp_device_sort_hashes(mirp_ctx* c, MirpHashRec* d, MirpHashRec* d_tmp, long long n, int bits);
// reads_kernels.hip: the read collapse of process-reads-fasta.py on a file held in host memory (out: the .processed text, malloc'ed)
int mirp_device_collapse_reads(mirp_ctx* c, const char* text, long long n, const char* prefix, int hash_bits, char** out, long long* out_len,
                               long long* n_reads, long long* n_unique, long long* bad_offset, double seconds[6]);
// align_kernels.hip: the alignment index and one batch of reads (mirp_align.cpp parses the files)
int mirp_device_align_index(mirp_ctx* c, const unsigned* pk, const unsigned* amb, const unsigned* cst, long long total,
                            const std::vector<unsigned long long>& cstart, const std::string& names, const std::vector<long long>& noff, double seconds[4]);
// the three steps of a batch, and the placement of multi-mapped reads between hits and emit (mirp_align_reads_placed)
int mirp_device_align_upload(mirp_ctx* c, const unsigned char* codes, const long long* roff, const char* qn, const long long* qoff, const unsigned* depth,
                             long long n, double seconds[5]);
int mirp_device_align_hits(mirp_ctx* c, long long n, int v, int m, int filter, const MirpAlignTailOpts* tail, long long* n_items, double seconds[6]);
int mirp_device_align_emit(mirp_ctx* c, long long n, long long n_items, int v, int k, int m, int filter, int place, const MirpAlignTailOpts* tail,
                           const std::function<int(const char*, size_t)>& sink, unsigned long long cnt[8], double seconds[6]);
// align_tail_kernels.hip: the 3' tails of the reads a batch left without a hit (mirp_align_reads_tailed), called from mirp_device_align_hits after
// the strata (counts, stratum, -m, slots, a_tt, the file's summary table) and after the items are allocated (the stratum's hits as items)
int mirp_device_align_tail_strata(mirp_ctx* c, long long n, const MirpAlignTailOpts& o, int m);
int mirp_device_align_tail_hits(mirp_ctx* c, const MirpAlignTailOpts& o);
// the summary table of a file: cleared before its first batch; after its last, rows = (tail letters, reads, depth) in (length, A < C < G < T < N) order
struct MirpTailRow { std::string tail; unsigned long long reads, depth; };
int mirp_device_align_tail_clear(mirp_ctx* c);
int mirp_device_align_tail_rows(mirp_ctx* c, std::vector<MirpTailRow>& rows);
int mirp_device_place_unique(mirp_ctx* c, long long n, long long* n_unique);
int mirp_device_place_prepare(mirp_ctx* c, long long n_unique, unsigned long long* depth_sum);
int mirp_device_place_pick(mirp_ctx* c, long long n, long long n_items, int mode, int window, unsigned long long seed, long long n_unique);
// reads_kernels.hip: the line split of an uploaded text shared by the collapse and the trim (starts[0 .. n_lines]); trim_kernels.hip: the trim of one FASTQ / FASTA text
int mirp_device_split_lines(mirp_ctx* c, const unsigned char* d_text, long long n, long long max_lines, DevBuf& tile_cnt, DevBuf& tile_scan, DevBuf& starts,
                            unsigned long long* d_first_bad, long long* n_lines, long long* bad_offset);
// the trim's steps, shared with the library profile: upload + split + records of a text of n > 0 bytes into the context's t_* arrays, then
// trim_reads_kernel under o (t_flen; res = {first bad record key, reads per flag bit 0..5, workgroups per path}) with the refusals that need the reads' bytes
struct MirpTrimParsed {
    bool fq;                          // FASTQ: the reads lie in the text and t_qual holds the quality starts; FASTA: in the gathered buffer
    long long R, rem, n_lines;        // reads, the lines behind the last whole FASTQ record, lines
    const unsigned char *d_text, *d_base;   // the uploaded text; what t_src points into
};
int mirp_device_trim_parse(mirp_ctx* c, const char* text, long long n, const char* name, int quality_cutoff, MirpTrimParsed* p, double seconds[3]);
int mirp_device_trim_cut(mirp_ctx* c, const MirpTrimParsed& p, const char* name, const MirpTrimOpts& o, unsigned long long res[9]);
int mirp_device_trim_reads(mirp_ctx* c, const char* text, long long n, const char* name, const MirpTrimOpts& o,
                           const std::function<int(const char*, size_t)>& sink, long long stats[7], double seconds[6]);
// libqc_kernels.hip: the k-mer table, the adapter walk and the three tables of one FASTQ / FASTA text (mirp_libqc.cpp checks the arguments)
int mirp_device_libqc_reads(mirp_ctx* c, const char* text, long long n, const char* name, const MirpLibqcOpts& o, MirpLibqcFound* found, long long stats[4],
                            long long* raw_len, long long* cycles, long long* insert, double seconds[6]);
int mirp_device_libqc_table(mirp_ctx* c, unsigned* out);      // the 4^12 counters of the last profile, to the host
// targets_kernels.hip: the target-site search over packed targets (mirp_targets.cpp parses the files)
int mirp_device_target_scan(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                            const std::vector<unsigned long long>& cstart, const std::string& tnames, const std::vector<long long>& tnoff,
                            std::vector<TgMirna>& mi, const std::vector<unsigned char>& mcodes, const std::string& mnames, const std::vector<long long>& mnoff,
                            const MirpTargetOpts& o, const std::function<int(const char*, size_t)>& sink, long long stats[2], double seconds[4]);
// mimic_kernels.hip: the seed-anchored target-mimic search over packed targets (mirp_mimics.cpp parses the files and builds the seed table)
int mirp_device_mimic_scan(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                           const std::vector<unsigned long long>& cstart, const std::string& tnames, const std::vector<long long>& tnoff,
                           std::vector<TgMirna>& mi, const std::vector<unsigned>& mid, const std::vector<unsigned>& slot, const std::vector<unsigned>& start,
                           const std::vector<unsigned char>& mcodes, const std::vector<int>& mlens, const std::string& mnames, const std::vector<long long>& mnoff,
                           const MirpMimicOpts& o, const std::function<int(const char*, size_t)>& sink, long long stats[4], double seconds[4]);
// degradome_kernels.hip: the cleavage scan of the resident alignments against packed transcripts (mirp_degradome.cpp parses the files and writes the
// lines).  sqstart / sqlen: first packed position and length of the transcript of every SAM tid; f2s: FASTA index -> SAM tid (-1: no @SQ line);
// mi / mi_anchored: the masks of make_mirna without / with `anchored`.  Hits arrive at the sink in output order, pass by pass: key = miRNA index in
// its group of 2^16 << 40 | category << 37 | half-score << 32 | packed position of the cleavage base; sites[mloc * 17 + h] = N_m(h) and
// pval[(mloc * 5 + category) * 17 + h] belong to the group at mbase.  stats = {records, sense, minus-strand, units, C_0 .. C_4, evaluations, hits,
// passes}; seconds = {upload, units + categories + windows, site counts, anchored counts, key passes + sort + download + write}.
struct MirpDgHit { unsigned long long key, reads, tmax; };
typedef std::function<int(int mbase, const MirpDgHit* hits, size_t n, const unsigned long long* sites, const double* pval)> MirpDgSink;
int mirp_device_degradome(mirp_ctx* c, const unsigned long long* pk, const unsigned* amb, const unsigned* cst, long long total,
                          const std::vector<unsigned long long>& cstart, const std::vector<int>& f2s, const std::vector<unsigned long long>& sqstart,
                          const std::vector<long long>& sqlen, std::vector<TgMirna>& mi, std::vector<TgMirna>& mi_anchored, int max_half, int max_cat, double alpha,
                          const MirpDgSink& sink, long long stats[12], double seconds[6]);
// annotate_kernels.hip: the comparison of packed queries with packed known sequences (mirp_annotate.cpp parses the files and writes the lines).
// AnPacked: position i's 2-bit code (A C G U = 0..3, 0 where unknown) at bits 2 i of `word`, bit i of `unk` set where unknown, `len` 12..32.
// hits_per_query is filled (hits before the -k cut) before the first sink call.  Kept keys arrive at the sink in output order, group by group:
// key = query index - qbase << 35 | distance << 31 | mismatches << 28 | known index << 4 | shift + 4.  stats = {hits, keys kept, passes};
// seconds = {upload, counting scan, key scans, sort + cut, download + write}.
struct AnPacked { unsigned long long word; unsigned unk; int len; };
typedef std::function<int(long long qbase, const unsigned long long* keys, size_t n)> MirpAnSink;
int mirp_device_annotate(mirp_ctx* c, const std::vector<AnPacked>& q, const std::vector<AnPacked>& k, int max_offset, int max_mismatches, long long max_lines,
                         std::vector<unsigned>& hits_per_query, const MirpAnSink& sink, long long stats[3], double seconds[5]);
// randfold_kernels.hip: the shuffles and the statistics of one pass (mirp_randfold.cpp plans the passes).  The sequences stand in the order d_perm
// (position -> index in the call), d_cum[position] = letters before it; every sequence has jps consecutive jobs, with has_native the first one is
// the sequence itself; job j's row starts at d_cum[j / jps] * jps + (j % jps) * len.  shuffle: jobs [j0, j0 + n_jobs) -> rows at d_out + row - base
// and d_out_offs[0 .. n_jobs]; d_slab: as many bytes as d_out (dinucleotide only).  stats: the MFEs of those jobs into the records.
struct RfPlan {
    const unsigned char* d_codes; const long long* d_offs; const int* d_perm; const long long* d_cum;
    long long jps, k_first; int has_native, dinucleotide; unsigned long long seed;
};
void mirp_device_rf_shuffle(mirp_ctx* c, const RfPlan& p, long long j0, int n_jobs, long long base, unsigned char* d_out, long long* d_out_offs,
                            unsigned char* d_slab);
void mirp_device_rf_stats(mirp_ctx* c, const RfPlan& p, long long j0, int n_jobs, const int* d_mfe, const int* d_status, MirpRandfoldRec* d_rec, int* d_bad);
// duplex_kernels.hip: the two-strand fold of DESIGN.md §21, one wave per duplex; results per job: mfe (0.01 kcal/mol, 0 = unbound) and the 64-bit masks
// of the paired positions of a and b.  pairs: strands as codes 0..4 (N A C G U) at d_a + d_aoff[q] .. d_aoff[q + 1], likewise b, every length
// 1..64 and at most max_la / max_lb; d_evals (optional) += loop evaluations.  perfect: miRNA q of the group (codes 0..3 = A C G U, 4 = unknown, 32
// per miRNA) against its reverse complement.  sites: the sorted keys of a pass of the target search (targets_kernels.hip; bulge: the --bulge key
// layout); a key that -k cuts (max_sites, d_emitted as site_kept of site_keys.h reads them) is not folded and gets mfe 0 and empty masks.
struct DxTargets {
    const unsigned long long* pk; const unsigned* amb; const unsigned char* mcodes; const TgMirna* mi; const unsigned long long* cstart;
    int n_contigs, mbase;
};
int mirp_device_duplex_pairs(mirp_ctx* c, const unsigned char* d_a, const long long* d_aoff, const unsigned char* d_b, const long long* d_boff, long long n,
                             int max_la, int max_lb, int* d_mfe, unsigned long long* d_ma, unsigned long long* d_mb, unsigned long long* d_evals);
int mirp_device_duplex_perfect(mirp_ctx* c, const unsigned char* d_mcodes, const TgMirna* d_mi, long long n, int* d_mfe, unsigned long long* d_ma,
                               unsigned long long* d_mb);
int mirp_device_duplex_sites(mirp_ctx* c, const DxTargets& T, bool bulge, const unsigned long long* d_keys, long long n, long long max_sites,
                             const unsigned long long* d_emitted, int* d_mfe, unsigned long long* d_ma, unsigned long long* d_mb);
// ensemble_kernels.hip: the inside / outside fold of DESIGN.md §23, one workgroup per job.  A job: the codes (N A C G U = 0..4) of its sequence at
// d_codes + code_off, its slab of mirp_ensemble_slab_doubles(n) doubles at d_slab + slab_off, its centroid text at d_texts + text_off, its rows of
// the pair counts at row_off + i, its record and MFE at index rec.  fold: jobs [0, n_ring) have at most MIRP_ENSEMBLE_RING_N nt (Qb's diagonals
// ringed in LDS), the longest of them max_ring_n; the others read them from the slab.  reduce: p into the slab, the record and the centroid text.  bpp: with d_out null the
// number of pairs with p >= cutoff per row, else the pairs themselves at d_row_at[row].
#define MIRP_ENSEMBLE_RING_N 300
struct EnJob { long long code_off, slab_off, text_off, row_off; int n, rec; };
size_t mirp_ensemble_slab_doubles(int n);
int mirp_device_ensemble_fold(mirp_ctx* c, const unsigned char* d_codes, const EnJob* d_jobs, int n_ring, int n_jobs, int max_ring_n, double* d_slab);
int mirp_device_ensemble_reduce(mirp_ctx* c, const EnJob* d_jobs, int n_jobs, double* d_slab, const int* d_mfe, MirpEnsembleRec* d_recs, char* d_texts);
int mirp_device_ensemble_bpp(mirp_ctx* c, const EnJob* d_jobs, int n_jobs, const double* d_slab, double cutoff, int* d_row_cnt, const long long* d_row_at,
                             MirpBpp* d_out);
// unpaired_kernels.hip: Z and Z_open of DESIGN.md §24, one wave per window of at most MIRP_UNPAIRED_MAX nt.  batch: window w = the codes (N A C G U =
// 0..4) at d_codes + d_offs[w] .. d_offs[w + 1] with the 1-based interval d_lo[w] .. d_hi[w]; the launch folds the n windows d_order[0 .. n), none
// longer than n_max, into d_recs[w].  mirp_unpaired_class(len): the n_max of the launch a window of that length belongs to.  sites: the sorted keys
// of a pass of the target search, as mirp_device_duplex_sites reads them; the window is the site's interval with `up` / `down` more bases towards
// the 5' / 3' end of the target strand, clipped to the contig; longest: the longest interval among the keys (at most 33); d_milli[key] = upe x 1000 rounded to nearest; a key that -k cuts is not folded and gets 0.
#define MIRP_UNPAIRED_MAX 128
int mirp_unpaired_class(int len);
int mirp_device_unpaired_batch(mirp_ctx* c, const unsigned char* d_codes, const long long* d_offs, const int* d_lo, const int* d_hi, const int* d_order,
                               long long n, int n_max, MirpUnpairedRec* d_recs);
int mirp_device_unpaired_sites(mirp_ctx* c, const DxTargets& T, bool bulge, const unsigned long long* d_keys, long long n, long long max_sites,
                               const unsigned long long* d_emitted, int longest, int up, int down, int* d_milli);
// hairpin_kernels.hip: the gapped local alignment of DESIGN.md §25.  Codes: A C G U = 0..3; an unknown letter is 4 in a query and 5 in a known
// sequence, so that it equals nothing.  Q: every query starts at a multiple of MIRP_HAIRPIN_STRIP in `codes` and is padded to one with 6; K: the
// known sequences back to back.  Out: the hits in output order (after the max_lines cut), their ops in forward order and the ops' offsets
// (hits + 1 entries); c->hp_per_query, c->hp_stats and c->hp_sec are filled.
struct HpSeqs {
    std::vector<unsigned char> codes;
    std::vector<long long> at;
    std::vector<int> len;
};
int mirp_device_hairpin(mirp_ctx* c, const HpSeqs& Q, const HpSeqs& K, const MirpHairpinOpts& o, std::vector<MirpHairpinHit>& hits, std::vector<char>& ops,
                        std::vector<long long>& ops_off);
// homolog_kernels.hip: the placements of coded queries (0..3 = A C G T at roff[0 .. nq]) in the resident alignment index as sorted keys
// (query << 35 | packed position << 3 | strand << 2 | mismatches); windows, fold and evaluation of a chunk of them
// inverted_kernels.hip: the inverted repeats of DESIGN.md §30.  G: the contigs as 4-bit codes (A C G T = 0..3, anything else and the padding 4),
// 16 to a 64-bit word; contig k starts at row pstart[k], a multiple of 16, its last base is row pend[k] - 1, and at least one padding row follows
// it; `rows` = pstart[n_contigs].  Out: the accepted repeats in output order with contig-local 1-based positions, their ops and the ops' offsets;
// c->iv_stats and c->iv_sec are filled.
struct IvGenome {
    std::vector<unsigned long long> words;
    std::vector<long long> pstart, pend;
    long long rows = 0;
};
int mirp_device_inverted(mirp_ctx* c, const IvGenome& G, const MirpInvertedOpts& o, std::vector<MirpInvertedRec>& recs, std::vector<char>& ops,
                         std::vector<long long>& ops_off);
// nats_kernels.hip: the complementary transcript pairs of DESIGN.md §36.  T: transcript s holds len[s] bases (0: skipped) whose codes stand at
// nibble pos[s] (a multiple of 16) of `fwd` (A C G T = 0..3, anything else and the padding 4) and, reverse-complemented, of `rc` (anything else and
// the padding 5), 16 codes to a 64-bit word, with MIRP_NATS_GAP padding nibbles before the first transcript and after every one; wseq[w] = the
// transcript of word w, -1 for padding.  Out: the regions in output order, their ops and the ops' offsets; c->nt_stats and c->nt_sec are filled.
#define MIRP_NATS_GAP 1024
struct NtSeqs {
    std::vector<unsigned long long> fwd, rc;
    std::vector<int> wseq, len;
    std::vector<long long> pos;
};
int mirp_device_nats(mirp_ctx* c, const NtSeqs& T, const MirpNatsOpts& o, std::vector<MirpNatsRec>& recs, std::vector<char>& ops, std::vector<long long>& ops_off);
int mirp_device_homolog_scan(mirp_ctx* c, const unsigned char* codes, const long long* roff, long long nq, int v, int max_placements,
                             std::vector<unsigned long long>& keys, long long stats[3]);
int mirp_device_homolog_eval(mirp_ctx* c, const unsigned long long* keys, long long n, int precursor_len, int max_lines, HmWin* win, HmEval* ev,
                             std::vector<char>& text, long long* text_off, long long stats[4], double seconds[3]);
int mirp_device_mask_alns(mirp_ctx* c, MirpAln* d_alns, MirpAln* d_tmp, long long* n_io, MirpAln* d_segs, MirpAln* d_segtmp, const int* d_owner, const int* d_seg_span,
                          long long* nseg_io,
                          const long long* d_rfirst, const int* d_rstart, const int* d_remax);

namespace mirp {
// mirp_dist.cpp: collectives on the context's communicator (no-ops / local copies without one)
int dist_all_counts(mirp_ctx* c, long long mine, std::vector<long long>& counts);
int dist_gatherv_bytes(mirp_ctx* c, const void* d_src, long long mine, int dst, void* d_dst, const std::vector<long long>& counts);
int dist_alltoallv_bytes(mirp_ctx* c, const void* d_send, const std::vector<long long>& send_off, const std::vector<long long>& send_cnt, void* d_recv,
                         const std::vector<long long>& recv_off, const std::vector<long long>& recv_cnt);
int dist_allgather_ll(mirp_ctx* c, const long long* mine, int n, std::vector<long long>& out);
int dist_agree(mirp_ctx* c, int local_rc, const char* what);
}  // namespace mirp

// mirp_fold.cpp: folds n_work device-resident windows (seqs / offs / lens as the kernels expect) into the given output buffers.  Uses the LDS-resident
// kernels when the span allows and re-runs the windows they flag (length, 16-bit range) with the generic kernel.
int mirp_run_fold(mirp_ctx* c, const unsigned char* d_seqs, const long long* d_offs, const int* d_lens, int n_work, int n_cap, int span,
                  int max_lines, int stride, MirpFoldLine* d_lines, char* d_ss, int* d_nlines, int* d_mfe, int* d_status);

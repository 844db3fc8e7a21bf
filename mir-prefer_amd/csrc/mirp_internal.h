// Internal declarations shared by the HIP kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "../../include/mirprefer.h"
#include "fold_params.h"

// One read of the read collapse (reads_kernels.hip): 64-bit content hash and the read's index in file order, sorted by the hash (sort_kernels.hip).
struct MirpHashRec { unsigned long long hash; unsigned idx, pad; };

// One strand of one miRNA in the target-site search (targets_kernels.hip): 32-bit masks over the window positions j = 0 .. L - 1.
// pl / ph: low / high bit of the 2-bit code of the Watson-Crick target base; unk: unknown miRNA letters; g1 / g2: miRNA G / U (G:U with target U /
// G); seed: miRNA positions 2..13; cleave: positions 10 and 11 under -c, else 0.
struct TgStrand { unsigned pl, ph, unk, g1, g2, seed, cleave, pad; };
// One miRNA, plus (s[0]) and minus (s[1]) strand; lmask = positions 0 .. L - 1; half-scores smin .. smax are reported in the current pass.
struct TgMirna { TgStrand s[2]; unsigned lmask; int L, smin, smax; };

// One placement of the homolog search after its evaluation (homolog_kernels.hip): n_structs structures in the window's list; best =
// index of the passing structure of lowest normalised energy, -1 = none; code = 0 with a best, else the get_maturestar_info code of the structure of
// lowest normalised energy, -1 = the list is empty; status 2 = a capacity of the launch was exceeded (the window is run again).  With a best: the
// star and the fold region (1-based, exclusive ends), the figures of the mature / star duplex, the line's energy and length, the structure's length.
// window of one placement: contig, [ws, we) and the interval [m0, m1) as 1-based contig coordinates with exclusive ends (the pipeline's), strand
struct HmWin { int tid, ws, we, m0, m1, strand, query, mm; };
struct HmEval { int n_structs, best, code, status, prime5, total_bps, total_dots, star_s, star_e, fold_s, fold_e, energy, line_len, ss_len; };

namespace mirp {

size_t fold_generic_lds_bytes(int n_cap, int max_lines);
size_t fold_generic_ws_slot_ints(int n_cap, int span);
void launch_fold_generic(hipStream_t stream, int grid, const FoldParams* P, const unsigned char* seqs, const long long* offs,
                         const int* lens, const int* work_list, int n_work, int span, int n_cap, int* ws, size_t ws_slot_ints, int max_lines,
                         int ss_stride, MirpFoldLine* out_lines, char* out_ss, int* out_nlines, int* out_mfe, int* out_status);

// fold185_kernel.hip: vienna-1.8.5 compatibility mode
size_t fold185_lds_bytes(int n_cap, int max_lines);
size_t fold185_ws_slot_ints(int n_cap, int span);
hipError_t launch_fold185(hipStream_t stream, int grid, const FoldParams185* P, const unsigned char* seqs, const long long* offs, const int* lens,
                          const int* work_list, int n_work,
                          int span, int n_cap, int* ws, size_t ws_slot_ints, int max_lines, int ss_stride, MirpFoldLine* out_lines, char* out_ss,
                          int* out_nlines, int* out_mfe, int* out_status);

// fold_dedup_kernels.hip: windows of one mirp_fold that repeat an earlier window byte for byte.  One device buffer holds everything at the byte
// offsets of its layout: the duplicate count, the table (keys, vals: `table` slots, a power of two), the duplicates per representative (n_dup), the
// hashes, the map (dup_of[w] = lowest r < w with the same length and bytes, or -1) and the lengths the fold reads (0 for a duplicate).
struct FoldDedupLayout { unsigned table; size_t total, keys, vals, n_dup, clear_bytes, hash, dup_of, fold_lens, bytes; };
FoldDedupLayout fold_dedup_layout(long long n_win);
hipError_t launch_fold_dedup_find(hipStream_t st, const unsigned char* seqs, const long long* offs, const int* lens, int n_win, int hash_bits, char* buf,
                                  const FoldDedupLayout& L);
// after the fold: summary, structure lines and structure text of every representative into its duplicates' slots
hipError_t launch_fold_dedup_copy(hipStream_t st, const int* dup_of, int n_win, int max_lines, int ss_stride, MirpFoldLine* lines, char* ss, int* nlines, int* mfe,
                                  int* status);
// *out (+)= the duplicates of the windows base + list[0 .. *list_len); with total_dst also *total_dst = *total_src.  One workgroup: the lists are short.
hipError_t launch_fold_dedup_count(hipStream_t st, const int* list, const unsigned* list_len, int base, const int* n_dup, unsigned* out, bool accumulate,
                                   const unsigned* total_src, unsigned* total_dst);

struct PredictCaps { int p_cap, s_cap, m_cap, l_cap; };   // pieces per line, structures per window, candidate matures per window, staged lines per window (predict_kernel.hip)
PredictCaps predict_default_caps(int max_lines, int ss_stride);
size_t predict_lds_bytes(int max_lines, int ss_stride);
size_t predict_lds_bytes(int max_lines, int ss_stride, PredictCaps caps);
size_t predict_lds_bytes_min(int max_lines, int ss_stride);          // without the staged text (which moves to global memory when it does not fit)
size_t predict_lds_bytes_min(int max_lines, int ss_stride, PredictCaps caps);
hipError_t launch_predict(hipStream_t stream, int grid, const MirpWindow* windows, int n_windows, const MirpMature* matures,
                          const MirpAln* alns, long long n_alns, const MirpFoldLine* lines, const char* ss, int ss_stride, int max_lines,
                          const int* n_lines, MirpPredictParams pp, MirpMirna* out, int* n_out, int* status, unsigned int* rcount = nullptr,
                          int* rpool = nullptr, unsigned int rcap = 0, int rstride = 0, const int* wsel = nullptr, int n_sel = 0,
                          const int* skip = nullptr, const int* wslot = nullptr, const PredictCaps* caps = nullptr, int* need = nullptr);
// launch + re-run of the windows that exceeded a capacity, with capacities sized for them (predict_kernel.hip)
int run_predict_launch(hipStream_t stream, int n_cu, const MirpWindow* windows, int n_windows, const MirpMature* matures, const MirpAln* alns, long long n_alns,
                       const MirpFoldLine* lines, const char* ss, int ss_stride, int max_lines, const int* n_lines, MirpPredictParams pp, MirpMirna* out, int* n_out,
                       int* status, unsigned int* rcount, int* rpool, unsigned int rcap, int rstride, const int* wsel, int n_sel, const int* skip, std::string* err,
                       int* need_buf = nullptr, long long* jobs_rec = nullptr);

// fold_lds_kernel.hip
size_t fold_lds_bytes(int max_lines);
size_t fold_lds_epilogue_bytes(int max_lines);
size_t fold_lds_slab_shorts(int n_cap);
#ifdef MIRP_DIAG
void fold_lds_epi_clocks_print();
#endif
int fold_lds_max_n();
int fold_lds_gen_wing_d();
int fold_lds_max_span();
// What the launches of one sub-batch (serial path) or chunk share.  Window w of it is window win_base + w of the call: offs, lens, the outputs and
// dense_list start at its first window, slabs and win_state at its place in the archive; ctl is its block of the control block (fold_ctl.h).
struct FoldLdsArgs {
    const FoldParams* P; const unsigned char* seqs; const long long* offs; const int* lens;
    int n_work, win_base, span;
    short* slabs; size_t slab_shorts; int* win_state;
    unsigned int* ctl; int* fallback_list; unsigned int* fallback_count;      // the fallback list and its length belong to the call
    MirpFoldLine* out_lines; char* out_ss; int* out_nlines; int* out_mfe; int* out_status;
    int max_lines, ss_stride;
    int* dense_list;
    int light_clocks; long long* dbg_cycles;      // diagnostics build only
};
// Once per context (it is bound to one device) and number of structure lines, before the first launch: the kernels' LDS limits, and the check that a
// CU holds two workgroups of the default model's candidate-pool pass (else a line on stderr and hipErrorLaunchOutOfResources).
hipError_t fold_lds_prepare(int max_lines);
// grid: CUs' worth of workgroups (the pass knows how many a CU holds).  The pool pass leaves the windows it cannot fold in the dense list; the dense
// pass folds that list, or every window without a pool pass before it.  A fill is the pool pass and the dense pass behind it, or the dense pass alone.
hipError_t launch_fold_lds_pool(hipStream_t stream, int model, int grid, const FoldLdsArgs& a);
hipError_t launch_fold_lds_dense(hipStream_t stream, int model, int grid, const FoldLdsArgs& a, bool every_window);
hipError_t launch_fold_lds_epilogue(hipStream_t stream, int model, int grid, const FoldLdsArgs& a);      // grid: workgroups
// Epilogue workgroups (fold_lds_epilogue_kernel at max_lines) that registers, wave slots and LDS let a CU hold beside two workgroups of the default
// model's candidate-pool pass (at most the number its LDS layout was made for), from the kernels' own attributes; 0 = none (the chunked fold then takes the serial path), < 0 = a HIP error.
int fold_lds_overlap_epi_wgs(int max_lines);

// candidate_kernels.hip
void launch_cov_scatter(hipStream_t st, const MirpAln* alns, long long n, const long long* goff, const long long* clen, int cutoff, int* diff_p, int* diff_m);
void launch_cov_unscatter(hipStream_t st, const MirpAln* alns, long long n, const long long* goff, const long long* clen, int* diff_p, int* diff_m);
long long cov_scan_tiles(long long gtot);
size_t run_start_bytes();
int cov_scan_tile_positions();
void launch_cov_maxlen(hipStream_t st, const MirpAln* alns, long long n, int* out);
size_t cov_fused_aux_bytes(long long gtot);
hipError_t launch_cov_scan_fused(hipStream_t st, const MirpAln* alns, long long n, int max_len /* longest record */, const long long* goff, const long long* clen, int n_contigs, void* aux, int* diff_p,
                                 int* diff_m, long long gtot, int cutoff, unsigned long long* stat_d, unsigned long long* stat_c, unsigned int* ticket, void* starts,
                                 long long starts_cap, MirpDepthPos* depth_out, long long depth_cap, long long* depth_gx, unsigned long long* totals);
void launch_cov_scan(hipStream_t st, const int* diff_p, const int* diff_m, long long gtot, int cutoff, unsigned long long* stat_d,
                     unsigned long long* stat_c, unsigned int* ticket, void* starts, long long starts_cap, MirpDepthPos* depth_out,
                     long long depth_cap, long long* depth_gx, unsigned long long* totals);
void launch_run_walk(hipStream_t st, const void* starts, long long n_runs, const int* diff_p, const int* diff_m, long long gtot, int cutoff,
                     const long long* goff, int n_contigs, int min_len, MirpPeak* runs, int* keep, int first_run_double);
void launch_depth_fix(hipStream_t st, MirpDepthPos* d, const long long* gx, long long n, const long long* goff, int n_contigs);
void launch_excl_scan(hipStream_t st, const int* in, long long* out, long long n);      // out[n + 1]; arrays beyond 16,384 elements: many-workgroup look-back scan
void release_scan_scratch(hipStream_t st);                                              // frees that scan's per-stream descriptors (before the stream is destroyed)
void launch_peak_compact(hipStream_t st, const MirpPeak* runs, const int* keep, const long long* kscan, long long n_runs, int n_contigs,
                         const int* order, long long* csq, long long* cdest, MirpPeak* peaks_sq, MirpPeak* peaks_sorted);
void launch_region_head(hipStream_t st, const MirpPeak* P, long long n, int max_gap, int* head);
void launch_region_first(hipStream_t st, const int* head, const long long* hscan, long long n, long long* rfirst);
void launch_region_count(hipStream_t st, const MirpPeak* P, const long long* rfirst, long long n_regions, const long long* clen, int L,
                         int* n_entries, int* is_locus, int* n_slots);
void launch_region_emit(hipStream_t st, const MirpPeak* P, const long long* rfirst, long long n_regions, const long long* clen, int L,
                        const long long* escan, const long long* lscan, const long long* sscan, MirpWindow* W, MirpLocus* loci, MirpPeak* wpeaks,
                        int* roles, int seq_stride);
void launch_window_payload(hipStream_t st, MirpWindow* W, long long n_windows, const MirpPeak* P, const MirpAln* alns, long long n_alns,
                           const unsigned char* genome, const long long* gboff, const long long* clen, double min_mature_depth, int wmax, char* seqs,
                           MirpMature* matures, long long* first_rec /* scratch, n_windows entries */, int* rt_out = nullptr);

}  // namespace mirp

/*
 * mirprefer.h -- C-ABI of libmirprefer.so: the MI355X (gfx950) replacement for the subprocess
 * boundary of miR-PREFeR's candidate -> fold -> predict hot path.
 *
 * The reference has no FFI; the boundary it crosses is `samtools depth | awk`, `samtools faidx`,
 * `samtools view` and `RNALfold -L` subprocesses.  Each entry point below
 * names the reference interface (file:line in /root/reference/miR_PREFeR.py, "MP") it replaces.
 *
 * Conventions: plain C types only; inputs are caller-owned and borrowed for the call; outputs are
 * library-owned host buffers released with mirp_free(); every function returns 0 on success and a
 * negative code on error, with text available from mirp_last_error(); one context per device,
 * calls on a context are not re-entrant, different contexts are independent.
 */
#ifndef MIRPREFER_H
#define MIRPREFER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mirp_ctx mirp_ctx;

/* One structure line of `RNALfold -L` output: "<ss> (<energy/100 %6.2f>) <start %4d>". */
typedef struct {
    int32_t start;   /* 1-based start column as RNALfold prints it */
    int32_t len;     /* strlen of the dot-bracket text (incl. dangle dots) */
    int32_t energy;  /* 0.01 kcal/mol */
    int32_t printed; /* 0 if RNALfold's containment rule suppresses the line */
} MirpFoldLine;

/* One ungapped alignment (`<len>M`), 16 bytes.  Arrays of these are sorted stably by (tid, pos) over the
 * sample-ordered concatenation: the order of the reference's combined sorted BAM (MP:667-713, 807-859). */
typedef struct {
    int32_t tid;      /* contig index in @SQ order (MP:500-509) */
    int32_t pos;      /* 1-based leftmost position */
    uint32_t depth;   /* N of the read id `sample_rA_xN` (MP:242-253) */
    uint16_t len;     /* read length */
    uint8_t strand;   /* 0 '+', 1 '-' (flag & 16, MP:1445) */
    uint8_t sample;   /* index into the sample-name list (MP:3300-3308) */
} MirpAln;

typedef struct { int32_t tid, pos, dp, dm; } MirpDepthPos;        /* one line of bam.depth.cut<CUT> (MP:946-949) */
typedef struct { int32_t tid, start, end, strand; } MirpPeak;      /* [start,end) 1-based; dict_contigs entry (MP:961) */
typedef struct { int32_t start, end, strand, depth; } MirpMature;  /* MP:1484; strand -1 = the (0,0,0,0) fallback (MP:1476) */
/* One FASTA entry handed to the folder (MP:1124-1142, 1184-1192). */
typedef struct {
    int32_t tid, ws, we, strand, loc_s, loc_e;
    int32_t tag;                       /* 0 / 1 = 'L' / 2 = 'R' (MP:1116-1120) */
    int32_t n_peaks; int64_t peak_off; /* header peak list */
    int32_t n_matures; int32_t pad0; int64_t mature_off;
    int64_t seq_off; int32_t seq_len; int32_t pad1;
} MirpWindow;
typedef struct { int32_t tid, start, end, n_windows; int32_t w[2][2]; int64_t peak_first; int32_t n_peaks; int32_t pad; } MirpLocus; /* dict_loci entry (MP:1312-1316) */

#define MIRP_MAX_SAMPLES 255     /* ALIGNMENT_FILEs of one run (MP:3300-3308 has no limit; a record's sample index is 8 bits wide) */
#define MIRP_MAX_MIRNA_PER_WINDOW 8
typedef struct { int32_t n_samples, min_mature_len, max_mature_len, allow_3nt, allow_no_star, minlen; } MirpPredictParams;
/* One entry of check_loci's `miRNAs` list (MP:2296-2343); the structure text is line `line` of the window's fold
 * output, characters [ss_off, ss_off+ss_len). */
typedef struct {
    int32_t window, tid, fold_s, fold_e, mat_s, mat_e, star_s, star_e, strand, has_star;
    int32_t line, ss_off, ss_len;
    int32_t reserved; /* imperfect-star flags (MP:2146-2162): bit0 'max_imperfect_star' key present, bits1-2 which+1, bit3 max > 0 */
    int32_t total_depth_mature, total_depth_star; /* the 64-bit sums the decision used, saturated at 2^31 - 1 */
} MirpMirna;

int mirp_create(int device, mirp_ctx** out);
void mirp_destroy(mirp_ctx* ctx);
const char* mirp_last_error(const mirp_ctx* ctx);
void mirp_free(void* p);
/* ABI version of this header; bumped on any signature change. */
int mirp_abi_version(void);

/*
 * Which RNALfold the fold entry points reproduce.  The reference runs whatever `RNALfold` is on PATH (MP:3053) and bundles two:
 * dependency/Mac/osx-10.9/RNALfold-2.1.2 (Turner-2004 parameters, dangles = 2: the default here, LDS-resident fast path) and
 * dependency/Linux/x64/RNALfold = ViennaRNA 1.8.5 (Turner-1999 parameters, dangles = 1, multi-component structure strings:
 * compatibility mode, one generic kernel).  Both are bit-exact against the respective binary.  Sticky per context.
 */
#define MIRP_FOLD_MODEL_VIENNA_212 0
#define MIRP_FOLD_MODEL_VIENNA_185 1
int mirp_set_fold_model(mirp_ctx* ctx, int32_t model);

/*
 * Replaces: `RNALfold -L <span>` on a FASTA chunk (MP:3047-3119, command MP:3053, consumer MP:1541-1599).
 * seqs: concatenated sequence bytes (any case, T or U); offsets[n_seqs+1]: byte offsets into seqs.
 * Out (library-owned): lines[n_seqs*max_lines], ss[n_seqs*max_lines*ss_stride] (NUL-terminated texts),
 * n_lines[n_seqs], mfe[n_seqs] (0.01 kcal/mol, RNALfold's final " (%6.2f)" line), status[n_seqs]
 * (0 ok, 1 = more than max_lines structures: the first max_lines are returned and n_lines holds the number the sequence needs,
 * <0 = error for that sequence).
 * Any span: up to 300 (and sequences up to 350 nt) on the LDS-resident kernels, beyond that -- PRECURSOR_LEN up to the reference's limit of 3000
 * (MP:167-184) -- on the generic kernels (tables in a global workspace).  Sequences longer than about 4,000 nt (LDS of one workgroup; 5,000 nt: the
 * 32-bit ranking of interior loops) are refused with -5 and a message, not truncated.
 */
int mirp_fold_batch(mirp_ctx* ctx, const char* seqs, const int64_t* offsets, int32_t n_seqs, int32_t span,
                    int32_t max_lines, MirpFoldLine** lines, char** ss, int32_t* ss_stride, int32_t** n_lines,
                    int32_t** mfe, int32_t** status);

/* The same fold, returning the per-sequence summary only (number of structure lines, minimum free energy, status): the structure text stays
 * on the device and no line is copied back.  mirp_last_fold_kernel_ms / mirp_last_fold_fallbacks then cover the whole call. */
int mirp_fold_batch_summary(mirp_ctx* ctx, const char* seqs, const int64_t* offsets, int32_t n_seqs, int32_t span, int32_t max_lines,
                            int32_t** n_lines, int32_t** mfe, int32_t** status);

/*
 * Replaces: the per-window loop of filter_next_loci / check_loci (MP:2350-2432, 2206-2347) with its two
 * `samtools view` subprocesses per window (MP:2002-2031), given the fold output of mirp_fold_batch.
 * Out: mirnas[n_windows*MIRP_MAX_MIRNA_PER_WINDOW] (first n_mirnas[w] valid per window; entry 0 is the one
 * the reference keeps, MP:2494), status[w] (0 ok, >0 capacity flag).
 */
int mirp_predict_batch(mirp_ctx* ctx, const MirpWindow* windows, int32_t n_windows, const MirpMature* matures, int64_t n_matures,
                       const MirpAln* alns, int64_t n_alns, const MirpFoldLine* lines, const char* ss, int32_t ss_stride,
                       int32_t max_lines, const int32_t* n_lines, const MirpPredictParams* params, MirpMirna** mirnas,
                       int32_t** n_mirnas, int32_t** status);

/* The same filter with the -d bookkeeping of check_loci (dict_why_not_miRNA_reasons, MP:2206-2347): besides the miRNA lists, one int32 record per
 * window and per evaluated (mature, structure) pair -- the get_maturestar_info code (MP:1876-1999) and the expression numbers of the pair; layout
 * and flags as documented at mirp_predict_reasons. */
int mirp_predict_batch_reasons(mirp_ctx* ctx, const MirpWindow* windows, int32_t n_windows, const MirpMature* matures, int64_t n_matures,
                               const MirpAln* alns, int64_t n_alns, const MirpFoldLine* lines, const char* ss, int32_t ss_stride,
                               int32_t max_lines, const int32_t* n_lines, const MirpPredictParams* params, MirpMirna** mirnas,
                               int32_t** n_mirnas, int32_t** status, int32_t** reasons, int64_t* n_reasons, int32_t* reasons_stride);

/* ------------------------------------------------------------------------------------------------
 * Device-resident pipeline: inputs are uploaded once, every stage leaves its results in HBM for the
 * next one, and only what a caller asks for is copied back.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t cutoff;         /* READS_DEPTH_CUTOFF (MP:91, awk rule MP:938, weight cap MP:735) */
    int32_t min_peak_len;   /* 19 (MP:3389, MP:956) */
    int32_t max_gap;        /* MAX_GAP (MP:92, MP:1263) */
    int32_t precursor_len;  /* PRECURSOR_LEN (MP:90, MP:1272-1300, RNALfold -L MP:3053) */
} MirpCandidateParams;

/* Genome: contigs in @SQ order, bytes as in the FASTA (case preserved), concatenated. Replaces `samtools faidx` (MP:1100-1105). */
int mirp_load_genome(mirp_ctx* ctx, int32_t n_contigs, const int64_t* contig_len, const uint8_t* seq_concat);
/* Alignments sorted as described at MirpAln. Replaces the prepare-stage BAMs (MP:772-874) as device-resident records. */
int mirp_load_alignments(mirp_ctx* ctx, const MirpAln* alns, int64_t n_alns);
/* Coverage segments of gapped alignments (records of the MirpAln layout, any order): `samtools depth` counts only the M / = / X bases of an
 * alignment (MP:937-941) while the read bookkeeping of the reference works on POS and len(SEQ).  Such an alignment is
 * one MirpAln record (POS, len(SEQ)) plus segments: strand bit 1 set = subtract the interval [pos, pos+len) (takes the record's own interval
 * back out), clear = add it (one per M / = / X block).  Replaces any segments loaded before; mirp_load_alignments clears them. */
int mirp_load_coverage_segments(mirp_ctx* ctx, const MirpAln* segs, int64_t n_segs);
/* Contig sharding across GPUs (one context per shard, whole contigs per shard): the strand vote of the reference double-counts the first
 * position of the first covered run of every contig except the very first run of the depth file (MP:905-906 + 926-929).  A shard whose first
 * covered contig is preceded, in @SQ order, by a covered contig held by ANOTHER shard sets this to 1 so that its first run is double-counted
 * as in the single-file run; default 0 (the context holds the whole genome). */
int mirp_set_contig_shard(mirp_ctx* ctx, int32_t preceded_by_coverage_elsewhere);
/* Window-level re-balancing of a sharded run (the reference fans PIECES of the candidate list out to its worker processes, not contigs:
 * /root/reference/miR_PREFeR.py:1329-1354, 2468-2480).  After mirp_candidate a rank that holds more windows than its share keeps the first
 * n_keep of them -- mirp_fold, mirp_predict, mirp_get_windows, mirp_get_fold and the text writers then see only those -- and ships the rest
 * to under-loaded ranks (host side: mir-prefer_amd/balance.py), which fold and filter them through mirp_fold_batch / mirp_predict_batch.
 * n_keep must not cut an L/R window pair.  The next mirp_candidate restores the full list. */
int mirp_limit_windows(mirp_ctx* ctx, int64_t n_keep);
/* The exclusive prefix sum every compaction of the candidate stage is built on (kept runs, region heads, window slots ...; the Python loops of
 * MP:877-962 and MP:1246-1371 append to lists instead): out[k] = in[0] + .. + in[k-1] for k = 0 .. n, host arrays in and out, computed on the
 * context's device by the kernels the stage uses (one workgroup up to 16,384 elements, a single-pass look-back scan beyond).  For tests. */
int mirp_excl_scan_i32(mirp_ctx* ctx, const int32_t* in, int64_t n, int64_t* out);
/* The stable device sort under the ingest, the read collapse, the align index and every key pass (sort_kernels.hip): a least-significant-digit
 * radix sort, 8 bits per pass, whole records moved; records whose sorted bits are equal keep their input order.  Three record types, each sorted
 * on the context's device and stream by the kernels the commands use, host arrays in and out (out may be in).  For tests.
 *   mirp_sort_alns     MirpAln by the key (uint32) tid << posbits | (uint32) pos, width posbits + tidbits; posbits and tidbits 0..32.
 *   mirp_sort_records  16-byte records {uint64 key; uint32 a, b} (MirpSortRec) by the low `bits` bits of key; a and b are payload.
 *   mirp_sort_u64      64-bit records by the bits [base, base + bits).
 * The passes are whole digits: a width that is not a multiple of 8 is rounded up, so the order is by the key bits [base, base + 8 * ceil(bits / 8))
 * (base = 0 for the first two; bits past 63 count as 0).  A caller whose width is not a multiple of 8 keeps the bits above it equal, or means
 * them.  Bits outside that range have no influence.  Refused with -1: n < 0, a null array with n > 0, a negative base or width, base + bits > 64
 * (posbits + tidbits > 64, posbits or tidbits > 32).  n = 0 and a width of 0 succeed and copy the input. */
typedef struct { uint64_t key; uint32_t a, b; } MirpSortRec;
int mirp_sort_alns(mirp_ctx* ctx, const MirpAln* in, int64_t n, int32_t posbits, int32_t tidbits, MirpAln* out);
int mirp_sort_records(mirp_ctx* ctx, const MirpSortRec* in, int64_t n, int32_t bits, MirpSortRec* out);
int mirp_sort_u64(mirp_ctx* ctx, const uint64_t* in, int64_t n, int32_t base, int32_t bits, uint64_t* out);
/* Replaces gen_contig_typeA + gen_candidate_region_typeA + dump_loci_seqs_and_alignment_multiprocess
 * (MP:877-962, 1246-1371, 1065-1244). contig_order = contig indices in the order sorted(dict_contigs) visits them (MP:1309). */
int mirp_candidate(mirp_ctx* ctx, const MirpCandidateParams* params, const int32_t* contig_order, int64_t* n_peaks, int64_t* n_loci,
                   int64_t* n_windows);
/* Thresholded depth lines of `samtools depth | awk` (MP:937-949), on demand (checkpoint artefact). */
int mirp_get_depth(mirp_ctx* ctx, MirpDepthPos** depth, int64_t* n_depth);
/* dict_contigs (MP:961) in @SQ order. */
int mirp_get_peaks(mirp_ctx* ctx, MirpPeak** peaks, int64_t* n_peaks);
/* dict_loci (MP:1312-1316) + the peaks array (sorted-contig order) its peak_first/n_peaks index. */
int mirp_get_loci(mirp_ctx* ctx, MirpLocus** loci, int64_t* n_loci, MirpPeak** peaks_sorted, int64_t* n_peaks);
/* FASTA entries + alndump payload (MP:1124-1142, 1137): windows, their header peak lists, matures and sequences
 * (seqs[window.seq_off .. +seq_len)). wpeaks/matures are slot arrays indexed by peak_off / mature_off. */
int mirp_get_windows(mirp_ctx* ctx, MirpWindow** windows, int64_t* n_windows, MirpPeak** wpeaks, int64_t* n_wpeaks, MirpMature** matures,
                     int64_t* n_matures, char** seqs, int64_t* n_seq_bytes);
/* Inspection copy of the per-position read table of gen_loci_alignment_info (MP:1395-1468) that the candidate stage keeps in LDS only: for every
 * window and start position ws + x, x in [0, width), of the window's own strand {length of the most abundant read, its depth, total depth}
 * (first-seen maximum, MP:1457), table[(w*width + x)*3 + k]; zeros where no read starts. */
int mirp_get_window_readtable(mirp_ctx* ctx, int32_t** table, int32_t* width, int64_t* n_windows);
/* Replaces run_fold's RNALfold subprocesses (MP:3047-3119) for the resident windows.  max_lines is the structure-line capacity of the main
 * output buffers; RNALfold itself has no limit (MP:3053), so the windows that produce more lines (tandem repeats) are folded again, alone, at the
 * capacity no window can exceed, into side buffers (mirp_get_fold_overflow) that mirp_predict and mirp_write_fold_text read for those windows. */
int mirp_fold(mirp_ctx* ctx, int32_t span, int32_t max_lines);
/* Fold output of the resident windows, same layout as mirp_fold_batch. */
int mirp_get_fold(mirp_ctx* ctx, MirpFoldLine** lines, char** ss, int32_t* ss_stride, int32_t* max_lines, int32_t** n_lines, int32_t** mfe,
                  int32_t** status);
/* The windows of the last mirp_fold that needed more than max_lines structure lines: windows[n] (indices into the window list), their complete
 * output lines[n*max_lines2], ss[n*max_lines2*ss_stride], n_lines[n].  The slots of these windows in mirp_get_fold hold their first max_lines lines only;
 * n_lines / mfe / status of mirp_get_fold(_summary) are the ones of the complete run. */
int mirp_get_fold_overflow(mirp_ctx* ctx, int32_t** windows, int64_t* n, MirpFoldLine** lines, char** ss, int32_t* ss_stride, int32_t* max_lines2,
                           int32_t** n_lines);
/* Per-window summary of the resident fold output (no structure text): n_lines, mfe, status as in mirp_fold_batch. */
int mirp_get_fold_summary(mirp_ctx* ctx, int32_t** n_lines, int32_t** mfe, int32_t** status, int64_t* n_windows);
/* Writes the fold stage artefact `<prefix>_rnalfoldoutput_<i>` in RNALfold's own text format (MP:3085-3098; consumed by MP:1541-1599):
 * for every resident window the `>` header line taken from fasta_path (the candidate stage's FASTA), the printed structure lines
 * "%s (%6.2f) %4d", the upper-cased T->U sequence and " (%6.2f)". */
int mirp_write_fold_text(mirp_ctx* ctx, const char* fasta_path, const char* out_path);
/* The same file, written behind the caller: the call returns once the fold output has been copied off the device; formatting and writing run in
 * worker threads on host copies only, so the next stage (mirp_predict) may start.  mirp_wait_text joins every pending writer of the context and
 * returns the first error (mirp_destroy waits too). */
int mirp_write_fold_text_async(mirp_ctx* ctx, const char* fasta_path, const char* out_path);
int mirp_wait_text(mirp_ctx* ctx);
/* The candidate stage's text artefacts, formatted by native worker threads from the resident state (contig_names: n_names NUL-terminated names
 * back to back, @SQ order): the thresholded depth file `bam.depth.cut<CUT>` -- `chr\tpos\td+\td-` per position with d+ + d- > cutoff
 * (MP:937-949) -- and the folder's input FASTA `<prefix>.rnalfold.in_<i>.fa`: per resident window the header
 * `>chr:ws-we strand locS-locE {0|L|R} s,e,strand;... M:s-e/strand/depth ...` and the sequence (MP:1124-1142, 1162-1178). */
int mirp_write_depth_text(mirp_ctx* ctx, const char* path, const char* contig_names, int32_t n_names);
int mirp_write_window_fasta(mirp_ctx* ctx, const char* path, const char* contig_names, int32_t n_names);
/* Replaces gen_miRNA_loci_nopredict (MP:2435-2502) for the resident windows: per-window check_loci, the 0/(L,R) pairing
 * of filter_next_loci (MP:2373-2432) and the "first mature only" rule (MP:2494).  Out: result[n_result] in window order,
 * ss_text[n_result*ss_stride] NUL-terminated structure strings, n_passed[n_windows] = len(miRNAs) per FASTA entry, status[n_windows] = 0 or the
 * capacity flag of the filter kernel (2: more structure pieces than its table holds, 3: more candidate matures than its table holds): a caller
 * must treat a non-zero status as an error, the window's candidates were truncated. */
int mirp_predict(mirp_ctx* ctx, const MirpPredictParams* params, MirpMirna** result, int64_t* n_result, char** ss_text, int32_t* ss_stride,
                 int32_t** n_passed, int32_t** status, int64_t* n_windows);
/*
 * -d mode (OUTPUT_DETAILS_FOR_DEBUG): why a region is not reported, replaces the dict_why_not_miRNA_reasons bookkeeping of check_loci
 * (MP:2206-2347) that convert_failure_reasons_list / write_dict_reasons (MP:2505-2567) print.  Returns int32 records of `stride` ints:
 * one per window {window, -1, n_structures, any mature in [min,max], n_passed, 0...} and one per evaluated (mature, structure) pair
 * {window, mature index, structure index, line, ss_off, ss_len, get_maturestar_info code (0 ok, 1..12 = MP:1876-1999's failures),
 *  flags, fold_s, fold_e, star_s, star_e, depth on this strand, antisense, mature, isoform, star, imperfect star[3],
 *  mature-star distance, mature depth per sample[n_samples]};  flags: 1 mature/star too close, 2 star but too few reads on the duplex,
 *  4 no star and ALLOW_NO_STAR_EXPRESSION off, 8 too many start positions, 16 mature+iso ratio < 0.8, 32 mature depth <= 100,
 *  64 not expressed in all samples, 128 passed, 256 no read on the precursor.  Record order is unspecified (sort by the first three fields).
 * The flags follow the 64-bit depth sums; the depth fields of a record (depth on this strand .. imperfect star[3]) saturate at 2^31 - 1, as
 * MirpMirna's two totals do, and do not wrap.
 */
int mirp_predict_reasons(mirp_ctx* ctx, const MirpPredictParams* params, int32_t** records, int64_t* n_records, int32_t* stride);
/* Per-stage device time of the last mirp_candidate / mirp_fold / mirp_predict calls, measured with HIP events on the
 * context's stream: ms[0]=coverage scatter+scan, ms[1]=rest of candidate, ms[2]=fold kernel, ms[3]=predict kernel. */
int mirp_last_timings(mirp_ctx* ctx, double ms[4]);
/* Number of windows of the last fold call that the LDS-resident kernel handed to the generic kernel (window longer than 350 nt,
 * or energies outside the fast path's 16-bit ranges); purely informational -- results are identical either way. */
int64_t mirp_last_fold_fallbacks(mirp_ctx* ctx);
/* Number of windows of the last mirp_fold that needed more than max_lines structure lines and were folded again at full capacity. */
int64_t mirp_last_fold_overflow(mirp_ctx* ctx);
/* Which way the last coverage pass (mirp_candidate / mirp_get_depth) took: 1 = the scan built every tile's difference values from the sorted
 * records in LDS (dense inputs without coverage segments), 0 = atomic scatter into the dense difference arrays; informational, the results are
 * identical (the `samtools depth` replacement, /root/reference/miR_PREFeR.py:877-949). */
int mirp_last_coverage_fused(mirp_ctx* ctx);
/* Pins the coverage path of the following mirp_candidate / mirp_get_depth calls: -1 = picked by record density (default), 0 = atomic scatter,
 * 1 = fused scan whenever the input allows it (no coverage segments, no record longer than a scan tile).  For tests and measurements. */
int mirp_set_coverage_path(mirp_ctx* ctx, int32_t mode);
/* Pins how the fill kernel of the following folds relaxes the multiloop splits: 0 = over split candidates (default; a window whose
 * candidate pool overflows is folded by the dense kernel), 1 = the dense loop for every window.  The tables, and therefore every output, are
 * identical either way (RNALfold's DML minimum, /root/reference/miR_PREFeR.py:3053); for tests and measurements. */
int mirp_set_fold_split_path(mirp_ctx* ctx, int32_t mode);
/* Number of windows of the last fold call that the candidate-pool pass handed to the dense fill kernel (pool overflow or no room for a pool). */
int64_t mirp_last_fold_dense(mirp_ctx* ctx);

/* Fold overlap: a batch of the default model is folded in chunks of windows, the epilogue kernel of a chunk (exterior sweep, enumeration,
 * backtracks: it waits on memory) on a second stream beside the fill kernel of the next chunk (it computes out of LDS).  chunk_windows = -1:
 * automatic (default; batches of at least 8 rounds of the fill grid in chunks planned by fold_overlap_plan.h, smaller ones serially), 0: off, the serial path, N > 0: chunks of
 * N windows whatever the batch size.  Every output is identical either way.  vienna-1.8.5, mirp_set_fold_split_path(1), spans outside the
 * LDS-resident kernels and a device whose resources leave no room for an epilogue workgroup beside the fill always take the serial path. */
int mirp_set_fold_overlap(mirp_ctx* ctx, int32_t chunk_windows);
/* How the fills of a chunked fold are scheduled.  mode = -1: automatic (default: tail-free wherever the overlap runs), 1: tail-free, 0: ordered.
 * Tail-free: the fill of chunk k runs on stream k % 2 and does not wait for the fill before it, so the workgroups of the next fill take the places of
 * those that run out of windows and no CU idles at a chunk boundary; a chunk launches the candidate-pool pass only, and the windows handed to the
 * dense fill kernel (none on ordinary inputs) are folded chunk by chunk behind the last epilogue.  Ordered: every fill on the context's stream in
 * order, each followed by its dense pass.  Every output, mirp_last_fold_dense and mirp_last_fold_fallbacks are identical either way. */
int mirp_set_fold_overlap_tailfree(mirp_ctx* ctx, int32_t mode);
/* Chunks the last fold call ran in (0: the serial path). */
int mirp_last_fold_overlap_chunks(mirp_ctx* ctx);
/* Windows whose slabs (three 16-bit triangles per window) the following folds hold on the device at once.  windows = 0: the default, 8 GiB of slabs;
 * N > 0: at most N windows, never more than the default: the serial path folds sub-batches of N windows one behind the other, a slot of the chunked
 * fold's ring of three holds max(1, N / 3).  Every output, mirp_last_fold_dense and mirp_last_fold_fallbacks are identical whatever is set; lowered
 * only to test the sub-batch path and small ring slots.  A negative value returns -1. */
int mirp_set_fold_capacity(mirp_ctx* ctx, int64_t windows);
/* Fold dedup (mirp_fold only): a window whose bytes repeat an earlier window of the list is not folded; it gets that window's n_lines, mfe, status,
 * structure lines and text.  The candidate stage writes the left window of a short two-strand locus twice (MP:1184-1192), and repeats of the genome
 * give equal windows at other coordinates.  Raw bytes are compared (no case or T/U folding: a soft-masked copy is folded on its own), after a 64-bit
 * hash picks the candidate: a hash collision can leave a duplicate unmerged, never merge different windows.  on = 1 (default) / 0: every window is
 * folded, exactly as before.  Every output, mirp_last_fold_fallbacks, mirp_last_fold_dense and mirp_last_fold_overflow are identical either way (a
 * duplicate counts as its representative does).  mirp_fold_batch, mirp_ensemble, mirp_randfold and mirp_homolog_scan fold every sequence they are
 * given. */
int mirp_set_fold_dedup(mirp_ctx* ctx, int32_t on);
/* Duplicates the last mirp_fold skipped (0 with dedup off). */
int64_t mirp_last_fold_duplicates(mirp_ctx* ctx);
/* The map of the last mirp_fold: dup_of[w] = the lowest window index r < w with the same length and bytes as window w if w was skipped, else -1
 * (all -1 with dedup off).  The same on every run.  Free with mirp_free. */
int mirp_get_fold_duplicates(mirp_ctx* ctx, int32_t** dup_of, int64_t* n_windows);
/* For tests: the number of low bits of the dedup hash that count (0 = the default, all 64).  With a few bits different windows collide
 * everywhere: outputs stay identical, some duplicates are no longer found. */
int mirp_set_fold_dedup_hash_bits(mirp_ctx* ctx, int32_t bits);

/* Device time of the kernels of the last mirp_fold, HIP events: two numbers whose sum is the device time of the fold's main pass.  Serial path:
 * ms[0] = fill kernel(s) (fold_lds_kernel: the dynamic program), ms[1] = epilogue kernel(s) (exterior sweep, enumeration, backtracks), summed
 * over the sub-batches.  With fold overlap: ms[0] = from the first fill's start to the last fill's end, whichever stream that fill is on (ordered
 * schedule: dense passes included), ms[1] = the rest of the fold's device time: the part of the epilogues that no fill covers and, in the tail-free
 * schedule, the deferred dense passes with their epilogues, if any. */
int mirp_last_fold_kernel_ms(mirp_ctx* ctx, double ms[2]);
/* Measures the two roofs of the fold's fill kernel on this GPU with its own geometry (one 1024-thread workgroup per CU): out[0] ds_read_b32 and
 * out[1] ds_read_u16 wave-instructions per second (conflict-free, reads in flight), out[2] packed 16-bit add+min and out[3] 32-bit shift-add+min
 * VALU wave-instructions per second.  Measurement only; bench.py prices the fill kernel against them. */
int mirp_microbench(mirp_ctx* ctx, double out[4]);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: one process and one context per GPU, whole contigs per rank, no collective on the data path except
 * the ONE exchange step: the gather of the final loci list to rank 0 -- the analogue of the reference's `multiprocessing.Queue.put(list)` per
 * piece that the parent collects (MP:2461-2499) -- and, in the sharded ingest, the routing of parsed records to the rank that owns their contig
 * (mirp_ingest_sams_shard).  Both run over RCCL on the context's stream.  librccl.so.1 is resolved with dlopen at the first mirp_dist_* call: a
 * single-GPU run never loads it, and the process holds one HIP runtime and one RCCL instance (no torch type or torch communicator is involved;
 * the host binding only has to carry the 128-byte id from rank 0 to the other ranks, through a file or any CPU-side store).
 * ---------------------------------------------------------------------------------------------- */
#define MIRP_DIST_ID_BYTES 128
/* ncclGetUniqueId: called by one rank, the bytes are handed to every rank's mirp_dist_init. */
int mirp_dist_unique_id(uint8_t id[MIRP_DIST_ID_BYTES]);
/* ncclCommInitRank on the context's device (collective over all `world` ranks).  world = 1 is valid (every exchange is then a local copy). */
int mirp_dist_init(mirp_ctx* ctx, const uint8_t id[MIRP_DIST_ID_BYTES], int32_t rank, int32_t world);
/* The same rank / world bookkeeping without RCCL, for ranks that SHARE one GPU (RCCL refuses two ranks on one device): every exchange is staged
 * through the host and files in `dir`, a directory all ranks see.  For tests and for debugging a sharded run on a single-GPU machine. */
int mirp_dist_init_local(mirp_ctx* ctx, const char* dir, int32_t rank, int32_t world);
int mirp_dist_finalize(mirp_ctx* ctx);
int mirp_dist_rank(const mirp_ctx* ctx);
int mirp_dist_world(const mirp_ctx* ctx);
/* What RCCL reports about the context's communicator: info = {ncclCommCount, ncclCommUserRank, ncclCommCuDevice}; {-1, -1, -1} without a RCCL
 * communicator (one rank, or mirp_dist_init_local).  (The reference's pool has no analogue; it lets a scaling record prove N ranks on N devices.)
 * Every wait on a peer inside the mirp_dist_* / mirp_gather_* / mirp_exchange_bytes / mirp_ingest_sams_shard calls has a deadline of
 * MIRP_DIST_TIMEOUT_S seconds (environment, default 600): on expiry, or on an asynchronous RCCL error, the communicator is aborted (ncclCommAbort)
 * and the call -- and every later exchange on the context -- returns -7, where the reference's parent waits for ever on a crashed child
 * (result queue, MP:2461-2499). */
int mirp_dist_comm_info(mirp_ctx* ctx, int32_t info[3]);
/* Sum over the ranks of a small int64 vector, in place (n <= 1024); every rank gets the sums.  mirp_dist_barrier = one such reduction. */
int mirp_dist_allreduce_sum(mirp_ctx* ctx, int64_t* v, int32_t n);
int mirp_dist_barrier(mirp_ctx* ctx);
/* Replaces the result queue of gen_miRNA_loci_nopredict (MP:2461-2499): the result of the last mirp_predict of every rank (records + structure
 * text, as mirp_predict returns them), concatenated in rank order on rank dst straight from the device-resident arrays; n_result = 0 elsewhere.
 * tids are genome-wide contig indices on every rank, so the records need no translation. */
int mirp_gather_loci(mirp_ctx* ctx, int32_t dst, MirpMirna** result, int64_t* n_result, char** ss_text, int32_t* ss_stride);
/* The same gather for arbitrary fixed-size host records (per-rank counts may differ); out = NULL and n_out = 0 on ranks other than dst. */
int mirp_gather_records(mirp_ctx* ctx, const void* rec, int64_t n, int32_t rec_bytes, int32_t dst, void** out, int64_t* n_out);
/* All-to-all of host byte blocks on the context's communicator (RCCL grouped send / recv, staged through the device; the local transport for ranks
 * that share a GPU): send holds the blocks for rank 0 .. world-1 back to back, send_cnt[world] their sizes; *recv (mirp_free) receives the blocks
 * of rank 0 .. world-1 back to back, recv_cnt[world] their sizes.  Carries the window payloads of the re-balancing step (see mirp_limit_windows). */
int mirp_exchange_bytes(mirp_ctx* ctx, const void* send, const int64_t* send_cnt, void** recv, int64_t* recv_cnt);

/* ------------------------------------------------------------------------------------------------
 * Host-side native ingest (no device involved).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_contigs; char* contig_names;   /* n_contigs NUL-terminated names back to back, @SQ order of the first file (MP:500-509) */
    int64_t* contig_len;
    int32_t n_samples; char* sample_names;   /* one per SAM file (MP:3300-3308) */
    MirpAln* alns; int64_t n_alns;           /* stably sorted by (tid, pos) over the sample-ordered concatenation */
    MirpAln* segs; int64_t n_segs;           /* coverage segments of the gapped alignments (see mirp_load_coverage_segments), unordered */
} MirpSamData;
/* Replaces sam2bam / samtools cat / sort / expand_bamfile / strand split of prepare_data (MP:656-746, 772-874): parses the
 * sample SAM files (read ids `sample_rA_xN`) with n_threads threads (0 = all cores) and sorts on the host.  A record keeps POS and len(SEQ),
 * which is what the reference's read bookkeeping uses (MP:1439-1457, 2021); an alignment whose CIGAR is not `<len(SEQ)>M` also yields
 * coverage segments (`samtools depth` counts M / = / X bases only).
 * Returns 0 or -1 with a message in errbuf; release with mirp_free_sam_data. */
int mirp_ingest_sams(const char* const* paths, int32_t n_paths, int32_t n_threads, MirpSamData* out, char* errbuf, size_t errbuf_len);
void mirp_free_sam_data(MirpSamData* data);
/* One keep region of the GFF options as the reference's BED file has it (MP:543-652): contig index, 0-based half-open [start, end). */
typedef struct { int32_t tid, start, end; } MirpRegion;
/* The same ingest with the device doing the record work: host threads tokenize, the GPU applies the keep regions like `samtools view -L`
 * (MP:817-859; n_regions = 0: no filter) and sorts stably by (tid, pos) (LSD radix sort, ties keep sample-then-file order).  The sorted
 * records and segments stay resident as the context's alignments (as after mirp_load_alignments + mirp_load_coverage_segments) and are
 * returned in *out.  seconds (optional): {tokenize, upload + filter, sort, download}.  Errors: mirp_last_error. */
int mirp_ingest_sams_gpu(mirp_ctx* ctx, const char* const* paths, int32_t n_paths, int32_t n_threads, const MirpRegion* keep_regions,
                         int64_t n_regions, MirpSamData* out, double seconds[4]);

/* mirp_ingest_sams_gpu in two halves: the host half (header + threaded tokenizer; no context, so it can run while the device is still being opened) and the
 * device half (keep-region filter, stable (tid, pos) radix sort, the records resident as the context's alignments).  mirp_ingest_tokenized_gpu consumes and
 * releases `tokenized`; mirp_free_tokenized releases one that was never handed over.  Same results as mirp_ingest_sams_gpu (MP:772-874). */
int mirp_tokenize_sams(const char* const* paths, int32_t n_paths, int32_t n_threads, void** tokenized, char* errbuf, size_t errbuf_len);
int mirp_ingest_tokenized_gpu(mirp_ctx* ctx, void* tokenized, const MirpRegion* keep_regions, int64_t n_regions, MirpSamData* out, double seconds[4]);
void mirp_free_tokenized(void* tokenized);

/* The same ingest sharded over the ranks of the context's communicator (mirp_dist_init; without one, or with one rank, it equals
 * mirp_ingest_sams_gpu): every rank tokenizes its own byte range of every SAM file, the records are routed to the rank that owns their
 * contig -- owner_of_tid[n_contigs], the same whole-contig partition the later stages use -- with one all-to-all over RCCL, and every rank
 * filters and sorts what it owns.  Each rank's result is the (tid, pos)-stable subsequence of the single-process result for its contigs
 * (the blocks are laid out in file-then-offset order before the sort), so the two ingests are interchangeable.  Replaces the serial
 * prepare_data of the reference (MP:772-874). */
int mirp_ingest_sams_shard(mirp_ctx* ctx, const char* const* paths, int32_t n_paths, int32_t n_threads, const MirpRegion* keep_regions,
                           int64_t n_regions, const int32_t* owner_of_tid, MirpSamData* out, double seconds[4]);

/* FASTA file -> sequences (replaces the genome access of `samtools faidx`, MP:1100-1105; names are the first word of the header line as
 * faidx has them, bytes and case kept).  names: n_contigs NUL-terminated names back to back in file order; len[k] = length of sequence k or
 * -1 when it was not wanted; seq: the wanted sequences back to back (n_bytes).  want / n_want: keep only these names (n_want = 0: all). */
typedef struct { int32_t n_contigs; char* names; int64_t* len; uint8_t* seq; int64_t n_bytes; } MirpFastaData;
int mirp_read_fasta(const char* path, const char* const* want, int32_t n_want, MirpFastaData* out, char* errbuf, size_t errbuf_len);
void mirp_free_fasta_data(MirpFastaData* data);

/* Report side, host only: the bodies of the per-locus read-mapping files of gen_map_result (MP:2907-2959) -- per sample the
 * precursor with `total_mapped_reads=`, the structure, and every read of the locus' strand that lies inside the precursor laid out under it
 * (`m` / `s` padding and the [mature] / [star] marks for the exact mature / star reads) -- from the position-sorted records and the genome
 * instead of one `samtools view` + `samtools faidx` per locus.  loci[n][8] = {tid, fold_s, fold_e, mat_s, mat_e, star_s, star_e, strand};
 * ss = n NUL-terminated structure strings back to back; contig_seq[t] may be NULL for contigs this process does not hold (a locus there is
 * an error, -2); counts[n][n_samples] = reads on the precursor.  Out: text (bodies back to back) and offsets[n+1], released with mirp_free. */
int mirp_report_readmapping(const int32_t* loci, int64_t n_loci, const char* ss, const MirpAln* alns, int64_t n_alns, const uint8_t* const* contig_seq,
                            const int64_t* contig_len, int32_t n_contigs, const char* sample_names, int32_t n_samples, const int64_t* counts,
                            char** text, int64_t** offsets);


/* Report files of the predict stage, formatted and written by native threads, byte for byte what the reference writes:
 * <prefix>_miRNA.gff3 (gen_gff_from_result MP:2619-2641), _miRNA.mature.fa / _miRNA.precursor.fa / _miRNA.precursor.ss
 * (gen_mirna_fasta_ss_from_result MP:2963-3019), _miRNA.detail.csv (gen_csv_table MP:2744-2779), _miRNA.detail.html (gen_html_table_file
 * MP:2793-2904), miRNA.stat.txt (MP:3585-3593).  Host only (no device).  The loci are in their final order (resultlist.sort(), MP:2622):
 * loci[n][10] = {contig index, fold_s, fold_e, mat_s, mat_e, star_s, star_e, strand (0 '+', 1 '-'), star expressed (0 / 1), overhang
 * (0 "2:2", 1 "2:3", 2 "3:3")}; contig_names / ss / precursor / sample_names = NUL-terminated strings back to back (precursor = forward-strand
 * text chrom:fold_s-(fold_e-1), upper case, T -> U); counts[n][n_samples][4] = reads on precursor / mature / star / antisense region;
 * mirbase_form = four strings: what stands before and behind the mature sequence in the miRBase search form for taxon "Viridiplantae", then for
 * "ALL" (gen_search_miRBase_str MP:2773-2791).  A NULL path skips that file.  0 = ok, < 0 with a message in errbuf. */
int mirp_write_reports(int64_t n_loci, const int32_t* loci, const char* contig_names, int32_t n_contigs, const char* ss, const char* precursor,
                       const char* sample_names, int32_t n_samples, const int64_t* counts, const char* mirbase_form, const char* gff_path,
                       const char* mature_fa_path, const char* precursor_fa_path, const char* ss_path, const char* csv_path, const char* html_path,
                       const char* stat_path, char* errbuf, size_t errbuf_len);

/* Many small files at once -- the per-locus read-mapping files <folder>/miRNA-precursor_<k>.map.txt of gen_map_result (MP:2907-2959), one per
 * locus: paths = n NUL-terminated file names back to back, file k holds text[offs[k] .. offs[k+1]).  Creating thousands of files is system-call
 * time spent in the kernel's directory lock: n_threads <= 1 writes them with one native thread (the default of the Python host; 1 / 2 / 4 / 8 threads
 * measured the same on tmpfs and no better on an overlay file system), n_threads = k splits the list over k.  Host only.  0 = ok, -8 with the first
 * failing name in errbuf. */
int mirp_write_files(int64_t n_files, const char* paths, const char* text, const int64_t* offs, int32_t n_threads, char* errbuf, size_t errbuf_len);

/* The tail of run_predict in ONE call (MP:3545-3627; host only): from a result list as mirp_predict / mirp_gather_loci return it (records + structure
 * text rows of ss_stride bytes) to the readmapping/ folder and the seven report files under outdir.  Inside: the more abundant arm becomes the mature
 * (MP:2611-2617), the list is put in the order of resultlist.sort() (MP:2622: [chr, fold_s, fold_e, mat_s, mat_e, star_s, star_e, ss, strand, has_star],
 * element by element, stable), the per-sample read counts of gen_mirna_info (MP:2644-2728) are taken from the (tid, pos)-sorted records, then
 * mirp_report_readmapping + mirp_write_files (on a thread of their own) and mirp_write_reports do the formatting.  contig_seq[t] / contig_len[t] = the
 * bases of contig t on the host (NULL where not held: a locus there is an error).  Optional outputs (NULL to skip): order_out[n] = input index of
 * list position i, sorted_out[n] = the records in list order after the swap, counts_out[n][n_samples][4].  n = 0 writes nothing (the reference prints
 * "0 miRNA identified. No result files generated.", MP:3547-3550).  0 = ok, < 0 with a message in errbuf. */
int mirp_write_result_reports(const MirpMirna* result, int64_t n, const char* ss_text, int32_t ss_stride, const char* contig_names, int32_t n_contigs,
                              const uint8_t* const* contig_seq, const int64_t* contig_len, const MirpAln* alns, int64_t n_alns, const char* sample_names,
                              int32_t n_samples, const char* mirbase_form, const char* outdir, const char* prefix, int32_t* order_out,
                              MirpMirna* sorted_out, int64_t* counts_out, char* errbuf, size_t errbuf_len);

/* Window view: the fold and the filter (mirp_fold, mirp_predict, mirp_predict_reasons) run on windows [first, first + count) of the candidate stage's
 * list until the view is changed; count < 0 restores the whole list.  Window indices in the results are relative to `first`.  The getters and text
 * writers of the candidate stage are not affected by a view and must not be called while one is active.  (Analogue in the reference: the pieces
 * its folder and filter processes work through one after the other, MP:1329-1354, 2468-2480.) */
int mirp_select_windows(mirp_ctx* ctx, int64_t first, int64_t count);

/* The fold, the filter and the report files of a single-process run as ONE pipelined call (replaces run_fold + run_predict of the `pipeline` verb,
 * MP:3441-3627, when no stage artefact is to be kept): the window list is cut into about n_chunks chunks at places where the windows alone decide
 * the list order of the results (no window before the cut reaches the first window behind it, or the contig changes; an (L, R) pair is never split),
 * every chunk is folded and filtered (mirp_select_windows + mirp_fold + mirp_predict), and a host thread turns a chunk's loci into read-mapping files
 * (mirp_write_result_reports' steps) WHILE THE DEVICE FOLDS THE NEXT CHUNK; the seven report files follow at the end.  Arguments as
 * mirp_write_result_reports; max_lines as mirp_fold.  Out: n_loci, the number of chunks used, device_ms = {fold, filter} summed over the chunks.
 * Afterwards the context holds the whole window list again, without a fold (mirp_fold must run before any getter of the fold stage). */
int mirp_fold_predict_report_stream(mirp_ctx* ctx, int32_t span, int32_t max_lines, const MirpPredictParams* pp, int32_t n_chunks, const char* contig_names,
                                    int32_t n_contigs, const uint8_t* const* contig_seq, const int64_t* contig_len, const MirpAln* alns, int64_t n_alns,
                                    const char* sample_names, int32_t n_samples, const char* mirbase_form, const char* outdir, const char* prefix,
                                    int64_t* n_loci, int32_t* n_chunks_used, double device_ms[2]);

/* Read collapse of scripts/process-reads-fasta.py:60-80 (the step before the pipeline: the reads' ids carry their depth, `sample_rA_xN`, parsed
 * at MP:242-253) for one uncollapsed FASTA file: every line that does not start with '>' is a read, taken after str.strip(); lines end at \n, \r\n
 * or a lone \r (universal newlines); a blank line is the read "".  out_path receives ">" + prefix + "_r" + A + "_x" + B + "\n" + read + "\n" per
 * distinct read, A = 0, 1, ... in order of first occurrence (Python 3 dict order), B = its count.  Bytes >= 0x80 are refused (-9, the message
 * names the file and the byte's offset); more than 2^31 - 1 lines are refused.  hash_bits: width of the grouping hash, 64 on the product path
 * (smaller widths force collisions, which are resolved exactly).  Out: n_reads, n_unique, seconds = {read + upload, split, hash + sort,
 * verify + rank, emit + download, write}.  Nothing is written on error. */
int mirp_collapse_reads(mirp_ctx* ctx, const char* path, const char* prefix, const char* out_path, int32_t hash_bits, int64_t* n_reads,
                        int64_t* n_unique, double seconds[6]);
/* Reads of the last mirp_collapse_reads that lay in hash runs whose bytes differ (resolved on the host). */
int64_t mirp_last_collapse_collisions(const mirp_ctx* ctx);

/* Read alignment of scripts/bowtie-align-reads.py (`bowtie-build`, then `bowtie -v V --best --strata -k K -S`), with the semantics of DESIGN.md §12.
 * mirp_align_index parses the reference FASTA files paths[0 .. n_paths) in order (contig name = first word of the header; A C G T in either case are
 * bases, every other character is ambiguous and never aligned over), packs them 2-bit and builds the device-resident index, which every later
 * mirp_align_reads of this context uses until the next mirp_align_index.  Contigs of length 0 are dropped with a warning on stderr; duplicate or
 * empty names and 2^32 bases or more are refused (-10).  Out: n_contigs, total bases, seconds = {read + parse + pack, upload, keys, sort,
 * positions + buckets}. */
int mirp_align_index(mirp_ctx* ctx, const char* const* paths, int32_t n_paths, int32_t* n_contigs, int64_t* total, double seconds[5]);
/* Aligns the reads of one FASTA file (QNAME = first word of the header, multi-line sequences concatenated) with at most v (0..3) mismatches: only
 * the best stratum, and a read with more than m (> 0) hits there is reported unaligned with XM:i:<m+1> (m = 0: off); the first k hits in (contig,
 * offset, + before -) order.  Writes out_path: @HD, one @SQ per contig, @PG with CL:"<pg_cl>", one record per hit or unaligned read (filter_unmapped:
 * no unaligned records).  A read longer than 1,024 nt or more than 2^31 - 1 reads are refused (-10) before out_path is opened.  Out: stats =
 * {reads, aligned, unaligned, suppressed, records}, seconds = {read + parse, upload, seeds, verify, sort, emit + download + write}. */
int mirp_align_reads(mirp_ctx* ctx, const char* reads_path, const char* out_path, const char* pg_cl, int32_t v, int32_t k, int32_t m, int32_t filter_unmapped,
                     int64_t stats[5], double seconds[6]);
/* Batches the last mirp_align_reads of this context ran on the device (a file is cut into batches of at most 2^22 reads, fewer than 2^28 bases and
 * at most 2^26 seeds; 0 before the first call and for a file without reads). */
int64_t mirp_align_last_batches(const mirp_ctx* ctx);
/* Placement of multi-mapped reads (DESIGN.md §12 "Placement", ShortStack's --mmap u / r): every read gets one record.  mode 0: off; 1 (u): a read with
 * 2..m best-stratum hits goes to one of them with probability proportional to the depths of the uniquely mapped reads of this file that start within
 * `window` bases of the hit on its contig, or to a uniformly drawn hit where no hit has any; 2 (r): always the uniform draw.  The draw is a hash of
 * the read's bases xor `seed`. */
typedef struct {
    int32_t mode;                            /* 0 off, 1 u, 2 r */
    int32_t window;                          /* 0..10000 */
    uint64_t seed;
} MirpAlignPlaceOpts;
/* mirp_align_reads with placement.  place == NULL or mode 0: exactly mirp_align_reads.  Otherwise m must be 1..10000 (a read with more than m hits is
 * suppressed as in mirp_align_reads), k is not consulted, and the record of an aligned read carries NH:i:<hits> XY:Z:<N unique | U by density |
 * R at random> XW:Z:<weight of the chosen hit>/<sum of the weights> after NM:i:.  A file for which m * (total depth of its unique reads) is 2^63 or
 * more is refused (-10) before out_path is opened.  Out: stats = mirp_align_reads' five, then {unique, by density, at random}; seconds =
 * mirp_align_reads' six, then {unique list + sort + prefix + weights + picks, the whole first pass}. */
int mirp_align_reads_placed(mirp_ctx* ctx, const char* reads_path, const char* out_path, const char* pg_cl, int32_t v, int32_t k, int32_t m,
                            int32_t filter_unmapped, const MirpAlignPlaceOpts* place, int64_t stats[8], double seconds[8]);
/* The placement runs a file's batches twice: the first pass finds the unique reads of the whole file and keeps the sorted hits of the batches
 * resident (8 bytes a hit) up to `items` hits (0 = the default, 2^28); a batch that does not fit is aligned again in the second pass, with the same
 * output.  A file of one batch is never aligned twice. */
int mirp_set_align_place_capacity(mirp_ctx* ctx, int64_t items);
/* Batches the last mirp_align_reads_placed of this context aligned twice. */
int64_t mirp_align_place_last_realigned(const mirp_ctx* ctx);
/* 3' non-templated tails (DESIGN.md §12 "Tails"): a read of length L that mirp_align_reads leaves without a hit (not one suppressed by m) and with
 * L >= min_templated + 1 is searched for hits of its 5' m bases, L - min(max_tail, L - min_templated) <= m <= L - 1, that are exact, inside one
 * contig, free of ambiguous bases and maximal (the read base after the templated part does not continue the match).  The largest m over both
 * strands is the read's stratum; m (the option) and k apply to its hits as they do to end-to-end hits. */
typedef struct {
    int32_t max_tail;                        /* 0 off, 1..8 */
    int32_t min_templated;                   /* 12..1024 */
    int32_t trim;                            /* 1: SEQ and QUAL of a tailed record hold the templated part only, CIGAR <m>M */
    int32_t reserved;
} MirpAlignTailOpts;
/* mirp_align_reads with the tail search.  tail == NULL or max_tail 0: exactly mirp_align_reads, and tails_path is not touched.  Otherwise a tailed
 * record reads FLAG 0|16, POS = first templated base, CIGAR <m>M<t>S on + and <t>S<m>M on -, XA:i:0 MD:Z:<m> NM:i:0 XT:Z:<the read's last t letters
 * as sequenced>, and tails_path gets the summary of the file: a header `tail length reads depth` and one tab-separated row per tail string among the
 * reads reported as tailed (each read once; depth = the sum of the _x<N> of their names, 1 where there is none), ordered by (length, A < C < G < T
 * < N).  Options out of range are refused (-1) before anything is opened; on a later error both files are removed.  Out: stats =
 * mirp_align_reads' five, where aligned includes the tailed reads and suppressed those with more than m hits in their tail stratum, then {tailed,
 * suppressed in the tail pass}; seconds = mirp_align_reads' six, then the tail pass. */
int mirp_align_reads_tailed(mirp_ctx* ctx, const char* reads_path, const char* out_path, const char* tails_path, const char* pg_cl, int32_t v, int32_t k,
                            int32_t m, int32_t filter_unmapped, const MirpAlignTailOpts* tail, int64_t stats[7], double seconds[7]);

/* 3' adapter and quality trimming of raw reads, the step before mirp_collapse_reads.  adapter[0 .. adapter_len) = A C G T in either
 * case (adapter_len 0..64; 0 = no adapter search); error_permille 0..999 = E in per-mille (an overlap of length l allows floor(E * l / 1000)
 * mismatches); min_overlap 1..adapter_len; quality_cutoff 0..93 (0 = off; Phred+33, FASTQ only); reads shorter than min_length or, when max_length
 * > 0, longer than max_length after trimming are dropped, and with discard_untrimmed so are reads without an adapter match. */
typedef struct {
    char adapter[64];
    int32_t adapter_len, error_permille, min_overlap, quality_cutoff, min_length, max_length, discard_untrimmed, reserved;
} MirpTrimOpts;
/* Trims the reads of one FASTQ or FASTA text held in host memory (data[0 .. n), decompressed by the caller; name = what messages call the file) and
 * writes one FASTA record `>name\n<trimmed read>\n` per kept read to out_path, in input order.  The format is told by the first byte (@ or >).
 * Refusals, each before out_path is opened: a byte >= 0x80 (-9, the offset in mirp_last_error); a malformed FASTQ record, a read longer than
 * 1,024 nt or a name longer than 1,048,576 bytes (-10, the 1-based record in mirp_last_error); an unknown first byte, more than 2^31 - 1 reads
 * and quality_cutoff > 0 on FASTA (-10, whole-file refusals without a record).  On a refusal or a later error a file at out_path (also one left
 * by an earlier call) is removed.  Out: stats = {reads, quality-trimmed, with adapter, untrimmed discarded, too short, too long, written} (reads = the last four
 * summed), seconds = {upload, split, records, trim, emit + download, write}. */
int mirp_trim_reads(mirp_ctx* ctx, const char* data, int64_t n, const char* name, const MirpTrimOpts* opts, const char* out_path, int64_t stats[7],
                    double seconds[6]);
/* How the trim kernel of the last mirp_trim_reads of this context read its reads: out[0] = the workgroups (128 consecutive reads each) that
 * staged their reads' text in LDS, out[1] = those whose text is over 32 KiB and was read from device memory; a workgroup without a valid read
 * counts as neither.  Both are 0 after a call that was refused or failed.  No output depends on the path; the entry is there for tests.
 * Returns -1 without a context or out. */
int mirp_trim_last_paths(const mirp_ctx* ctx, int64_t out[2]);

/* Profile of a raw library, the step before mirp_trim_reads: its 3' adapter, found from the reads, and three tables.  adapter_len
 * 0 = find the adapter; 1..64 = use adapter[0 .. adapter_len) (A C G T in either case) for the insert table, the search still runs and is reported;
 * error_permille 0..999 as in MirpTrimOpts; min_overlap 0 = the trim's default (3), else 1..64, an overlap beyond the adapter in use counts as its
 * length; sample 1..2^26 = the reads, from the first on, whose 12-mers are counted. */
typedef struct {
    char adapter[64];
    int32_t adapter_len, error_permille, min_overlap, reserved;
    int64_t sample;
} MirpLibqcOpts;
#define MIRP_LIBQC_NONE 0    /* no eligible 12-mer occurs 16 times: no adapter, adapter_len 0 and the walk's fields 0 */
#define MIRP_LIBQC_OK 1      /* the left walk stopped where the 12-mers before the candidate are no longer one sequence: the adapter's start */
#define MIRP_LIBQC_UNSURE 2  /* the left walk ran out of support (1) or reached its cap of 1,024 (2): the candidate may be an abundant insert */
/* adapter[0 .. adapter_len) = the candidate in upper case (adapter_len 12..64, 0 with status NONE); seed_code = the seed 12-mer, 2 bits per base
 * (A 0, C 1, G 2, T 3), first base most significant; seed_count = its counter; min_count = max(16, seed_count / 64), the support a step needs;
 * left_steps = bases the left walk put before the seed; left_stop = 0 purity, 1 support, 2 the length cap. */
typedef struct {
    char adapter[64];
    int32_t adapter_len, status, seed_code, left_steps, left_stop, reserved;
    int64_t seed_count, min_count;
} MirpLibqcFound;
/* Profiles the reads of one FASTQ or FASTA text held in host memory (data[0 .. n), decompressed by the caller; name = what messages call the file).
 * The input rules and refusals are those of mirp_trim_reads with quality_cutoff 0, with the same codes and messages (-9, -10); nothing is written.
 * Every 12-mer of A C G T (after upper-casing) that lies within the first 64 bases of one of the first min(reads, sample) reads counts once in a
 * table of 4^12 32-bit counters; the adapter is walked out of that table by integer comparisons alone, so it does not depend on
 * the order the reads are counted in.  Out, over all reads: found; stats = {reads, sampled, with adapter, dimers}; raw_len[1025] = reads of each
 * length; cycles[1024][6] = per cycle the reads with A, C, G, T, anything else, and the sum of quality - 33 (0 for FASTA); insert[1025][6] = per cut
 * p of the trim's adapter step (opts' adapter, else the found one of status OK or UNSURE; error_permille and min_overlap; no quality trim, no
 * length filter; p = the read's length without a match) the reads whose first base is A, C, G, T, anything else (a read cut at 0, a dimer, counts
 * here), and their total; all zeros, as are with adapter and dimers, when there is no adapter to use.  with adapter = reads with a match, dimers
 * = those matched at 0.  seconds = {upload, split, records, k-mers + adapter, trim, tables}.  Any of the out pointers may be NULL.
 * mirp_trim_last_paths reports the trim kernel's paths of this call too. */
int mirp_libqc_reads(mirp_ctx* ctx, const char* data, int64_t n, const char* name, const MirpLibqcOpts* opts, MirpLibqcFound* found, int64_t stats[4],
                     int64_t raw_len[1025], int64_t cycles[1024 * 6], int64_t insert[1025 * 6], double seconds[6]);
/* Copies the 4^12 counters of the last mirp_libqc_reads of this context to out; -1 without a context or out, and after a call that was refused or
 * failed (or before the first call).  No output is read from it; the entry is there for tests. */
int mirp_libqc_last_table(mirp_ctx* ctx, uint32_t out[1 << 24]);

/* Plant miRNA target sites: every miRNA against every offset of every target, ungapped, scored by position-weighted mismatches
 * (mismatch 1, G:U 0.5, doubled at miRNA positions 2..13) in half-units.  max_half_score 0..16 (= 2 x the -s score); both_strands: also the minus
 * strand; cleavage_site: reject a site with a mismatch (not a G:U) at miRNA position 10 or 11; max_sites: the first N sites per miRNA in output
 * order (0 = all); bulge (0 or 1): also the sites with exactly one unpaired nucleotide, on the target (tP) or on the miRNA (mP), and a last
 * column `bulge` on every line (§14, "Bulged sites"); 0 leaves every byte of the output as it was.  energy (0 or 1): four more last columns on
 * every line, `mfe mfe_perfect mfe_ratio duplex` (§21, "targets -e"): the free energy of the duplex of the miRNA with the site and one flanking
 * base on each side (mirp_duplex_batch's fold, not forced onto the alignment of `pairs`), that of the miRNA with its reverse complement, their
 * ratio to three decimals (NA when the perfect duplex is unbound) and the structure text; 0 leaves every byte of the output as it was.
 * accessibility (0 or 1): a last column `upe` on every line (§24, "targets -u"): the energy in kcal/mol, to three decimals, that opens the site
 * inside its window of the target strand -- the site's interval and mirp_set_target_flanks' bases beside it, clipped to the contig
 * (mirp_unpaired_batch's upe of that window); 0 leaves every byte of the output as it was. */
typedef struct {
    int32_t max_half_score, both_strands, cleavage_site, bulge;
    int64_t max_sites;
    int32_t energy, accessibility;
} MirpTargetOpts;
/* Reads the miRNA FASTA mirna_path (name = the whole header after '>', stripped, tabs turned into spaces; multi-line sequences concatenated; A C G U T
 * in either case, T = U, any other letter unknown) and the target FASTA files target_paths[0 .. n_targets) (parsed and packed as mirp_align_index
 * does), and writes the TSV of §14 to out_path: a header line, then one line per site ordered by miRNA (file order), score, target (file order),
 * start, + before -, end.  Refusals, each before out_path is opened (-10, the 1-based record in mirp_last_error): a miRNA of length outside 12..32, an
 * empty name, a byte >= 0x80, more than 2^24 miRNAs; and the target refusals of mirp_align_index.  On any error the file at out_path is removed.
 * Out: stats = {miRNAs, targets, target bases, evaluations (offsets x miRNAs x strands), sites written, passes}, seconds = {parse, upload, scan,
 * sort + cut (with energy / accessibility: and the folds of the pass's keys), emit + download + write}. */
int mirp_target_scan(mirp_ctx* ctx, const char* mirna_path, const char* const* target_paths, int32_t n_targets, const MirpTargetOpts* opts,
                     const char* out_path, int64_t stats[6], double seconds[5]);
/* Keys (sites before the -k cut) one pass of mirp_target_scan holds on the device, at least 2; 0 = the default, 2^26.  A pass that finds more is
 * split into passes by (miRNA, score) and by ranges of offsets; lowered only to test that path.  With bulge a pass holds at least 4 keys whatever
 * is set here: the most one offset can hold of one miRNA and score (t and m on both strands), so that the split always ends. */
int mirp_set_target_capacity(mirp_ctx* ctx, int64_t keys);
/* Bytes of text that leave the device in one piece: the lines of a pass of mirp_target_scan and mirp_mimic_scan (whole lines per piece; a longer
 * line is a piece of its own) and the SAM / FASTA text of a batch of mirp_align_reads, mirp_align_reads_placed and mirp_trim_reads (cut at any
 * byte).  0 = the default, 1 GiB; negative values are refused (-1).  Lowered only to test the piece path; no output depends on it.
 * mirp_text_pieces_last: the non-empty pieces handed to the output by the last of those calls (the header lines a call writes itself are not
 * pieces); -1 without a context. */
int mirp_set_text_piece(mirp_ctx* ctx, int64_t bytes);
int64_t mirp_text_pieces_last(const mirp_ctx* ctx);

/* Endogenous target mimics: sites where a target pairs with a miRNA around a loop of loop_len unpaired target bases opposite the
 * gap between miRNA positions P and P + 1, P in {9, 10, 11}, so that the site cannot be sliced.  Positions 2..8 are Watson-Crick pairs, the pairs
 * P and P + 1 that close the loop are not mismatches, and imperfect = mismatches + G:U pairs over positions 1..L is at most max_imperfect; per
 * (miRNA, interval, strand) the P of lowest imperfect is written, the smallest on a tie.  max_imperfect 0..6; loop_len 2..6; both_strands (0 or 1):
 * also the minus strand; max_sites: the first N sites per miRNA in output order (0 = all). */
typedef struct {
    int32_t max_imperfect, loop_len, both_strands, reserved;
    int64_t max_sites;
} MirpMimicOpts;
/* Reads the miRNA FASTA and the target FASTA files exactly as mirp_target_scan does (same letters, same refusals) and writes the TSV of §27 to
 * out_path: a header line, then one line per site ordered by miRNA (file order), imperfect, target (file order), start, + before -.  The scan is
 * anchored on the seed: the 7-mer at every target position and strand selects, through a table of 16,384 buckets, the miRNAs whose positions 2..8
 * pair with it; a miRNA with an unknown letter in 2..8 is in no bucket and has no sites.  Passes hold at most mirp_set_target_capacity keys.  On any
 * error the file at out_path is removed.  Out: stats = {miRNAs, miRNAs without a usable seed, targets, target bases, seeds looked up (positions x
 * strands with a 7-mer of unambiguous bases inside one contig), bucket entries evaluated, sites written, passes}, seconds = {parse + table, upload,
 * scan, sort + cut, emit + download + write}.  Nothing resident changes. */
int mirp_mimic_scan(mirp_ctx* ctx, const char* mirna_path, const char* const* target_paths, int32_t n_targets, const MirpMimicOpts* opts,
                    const char* out_path, int64_t stats[8], double seconds[5]);

/* Phased siRNA (PHAS) windows on the context's resident alignments (after any SAM ingest, or after mirp_load_alignments).  A record
 * with len == length is a read of the unit (tid, strand, c), c = pos on the plus strand and pos + 2 on the minus strand (the 2-nt 3' overhang of a
 * Dicer duplex); its abundance is the sum of the records' depths, and units below min_depth are dropped first.  Every distinct (tid, c) of a unit is
 * an anchor x; its window [x, x + cycles * length) counts, over both strands, n units and k units with (c - x) % length == 0.  The window passes when
 * k >= max(kmin[n], min_phased).  length 1..1024, cycles 1..64, min_phased >= 1, min_depth >= 1; records with pos < 0 are ignored. */
typedef struct { int32_t length, cycles, min_phased, min_depth; } MirpPhaseOpts;
/* One passing window: contig, anchor x (1-based), n, k, and the abundance of its phased units and of all its units. */
typedef struct {
    int32_t tid, n, k, reserved;
    int64_t start, phased_reads, window_reads;
} MirpPhaseWindow;
/* kmin[0 .. 2 * cycles * length] is the caller's table (phasing.py computes it exactly from the hypergeometric p-value and alpha) and is only read.
 * Out: *windows (release with mirp_free) holds the *n_windows passing windows in (tid, start) order; stats (optional) = {records of length `length`,
 * units kept, anchors}.  Nothing resident changes. */
int mirp_phase_scan(mirp_ctx* ctx, const MirpPhaseOpts* opts, const int32_t* kmin, MirpPhaseWindow** windows, int64_t* n_windows, int64_t stats[3]);

/* miRNA triggers of PHAS loci on the context's resident alignments (after any SAM ingest, or after mirp_load_alignments).  Every
 * target site of a miRNA (§14 on both strands, score <= max_half_score / 2, no mismatch at miRNA position 10 or 11) that lies inside a locus
 * interval sets a cut, and the phasing test of §15 (units of `length`, `cycles`, min_depth) runs in the windows that the cut anchors: downstream
 * and upstream of the cut in transcript sense, each at the register offsets -drift .. drift.  A window with k >= max(kmin[n], min_phased) is a
 * trigger.  length 1..1024, cycles 1..64, min_phased >= 1, min_depth >= 1, max_half_score 0..16, drift 0..2. */
typedef struct { int32_t length, cycles, min_phased, min_depth, max_half_score, drift; } MirpTriggerOpts;
/* One locus interval, already widened by the flank and clipped to the contig: the tid of the resident alignments, the index of the same contig
 * in the genome files (file order), and [start, end], 1-based. */
typedef struct {
    int32_t tid, contig;
    int64_t start, end;
} MirpTriggerLocus;
/* One trigger: locus and miRNA (indices in the caller's order / the file), the site's half-score, strand (0 '+', 1 '-') and 0-based offset `pos` on
 * the contig, side (0 down, 1 up), the register offset, n, k and the abundance of the window's phased units and of all its units. */
typedef struct {
    int32_t locus, mirna, half, strand, side, offset, n, k;
    int64_t pos, phased_reads, window_reads;
} MirpTrigger;
/* Reads the miRNA FASTA and the genome FASTA files exactly as mirp_target_scan does (same letters, same refusals).  kmin[0 .. 2 * cycles * length]
 * is the caller's table, as for mirp_phase_scan.  Out: *triggers (release with mirp_free) holds the *n_triggers triggers ordered by locus, miRNA,
 * half-score, pos, strand, side, offset; site_counts[q] = the sites inside locus q's interval; stats (optional) = {miRNAs, interval bases, sites,
 * windows evaluated, records of length `length`, units kept}; seconds (optional) = {parse + pack, upload, site scan + sort, units, windows +
 * download}.  A bad argument (a null pointer, an option out of range, n_loci < 0, a locus with tid < 0, a contig that the genome files do not
 * hold, start < 1, start > end or end past the contig) is refused with -1 before anything is allocated on the device.  Nothing resident changes. */
int mirp_trigger_scan(mirp_ctx* ctx, const char* mirna_path, const char* const* genome_paths, int32_t n_genome, const MirpTriggerLocus* loci,
                      int64_t n_loci, const MirpTriggerOpts* opts, const int32_t* kmin, MirpTrigger** triggers, int64_t* n_triggers,
                      int64_t* site_counts, int64_t stats[6], double seconds[5]);

/* Small-RNA clusters on the context's resident alignments (after any SAM ingest, or after mirp_load_alignments).  A record spans
 * [pos, pos + len - 1]; coverage c(p) = the sum of the depths of the records whose span holds p, for p in 1..contig_len[tid] only (64-bit).
 * Islands are the maximal runs of c(p) >= threshold; islands of one contig whose gap (next start - end - 1) is <= pad merge into a cluster.
 * A record counts in the first cluster, in coordinate order, that its span overlaps, and in no other.  threshold >= 1, pad 0..10^6, n_samples
 * 1..255 (a counted record with sample >= n_samples is refused); records of a tid >= n_contigs cover nothing. */
typedef struct {
    int64_t threshold, pad;
    const int64_t* contig_len;      /* LN of contigs 0 .. n_contigs - 1 */
    int32_t n_contigs, n_samples;
} MirpClusterOpts;
/* One cluster: contig, [start, end] (1-based), depth sums, distinct (pos, strand, len) placements, the major placement (largest depth sum; ties
 * to the smallest pos, then + before -, then the shorter len; strand 0 '+', 1 '-') and the depth per size class. */
typedef struct {
    int32_t tid, major_strand, major_len, reserved;
    int64_t start, end, reads, plus_reads, placements, major_pos, major_reads;
    int64_t sizes[7];               /* len < 20, 20, 21, 22, 23, 24, > 24 */
} MirpCluster;
/* Out: *clusters (release with mirp_free) holds the *n_clusters clusters in (tid, start) order; *sample_counts (release with mirp_free) the depth
 * per (cluster, sample), n_clusters x n_samples, row-major; stats (optional) = {records, total depth, islands, clusters, records counted in a
 * cluster}.  Nothing resident changes. */
int mirp_cluster_scan(mirp_ctx* ctx, const MirpClusterOpts* opts, MirpCluster** clusters, int64_t* n_clusters, int64_t** sample_counts,
                      int64_t stats[5]);

/* Reads on given loci on the context's resident alignments (after any SAM ingest, or after mirp_load_alignments).  One locus:
 * contig, strand (0 '+', 1 '-', 2 none), [start, end] 1-based inclusive.  Its number is its index in the array.  (MirpLocus is the candidate
 * stage's dict_loci entry, hence the longer name.) */
typedef struct { int32_t tid, strand; int64_t start, end; } MirpLocusSpan;
typedef struct {
    const int64_t* contig_len;      /* LN of contigs 0 .. n_contigs - 1, each 0 .. 2^31 - 1 */
    int32_t n_contigs, n_samples, stranded, reserved;
} MirpLocusOpts;
/* Table rows (records, placements) one wave-job of the scan serves, and the most loci of a call.  For tests of the ranges around a multiple of
 * the chunk: no result depends on where a chunk ends. */
#define MIRP_LOCI_CHUNK 4096
#define MIRP_LOCI_MAX 16777216
/* A record's span is mirp_cluster_scan's, [max(pos, 1), min(pos + len - 1, LN)]; a record with an empty span or a tid >= n_contigs counts
 * nowhere.  A record counts in every locus of its contig whose [start, end] shares a position with its span -- the loci may overlap, nest and
 * repeat -- and, with `stranded`, only in loci of its own strand or of none.  Per locus the sums of MirpCluster over the records it counts, all
 * 64-bit.  n_samples 1..255 (a counted record with sample >= n_samples is refused).  A bad argument (a null pointer, n_loci outside 0 .. 2^24,
 * n_samples out of range, a contig length outside 0 .. 2^31 - 1, a locus with a tid outside the table, a strand outside 0..2, start < 1,
 * start > end or end > LN) is refused with -1 before anything is allocated on the device.
 * Out: *out (release with mirp_free) holds one MirpCluster per locus in input order, tid, start and end echoed, everything else zero for a
 * locus that counts no record; *sample_counts (release with mirp_free) the depth per (locus, sample), n_loci x n_samples, row-major; stats
 * (optional) = {records, loci, (locus, chunk of records) jobs, (record, locus) pairs counted, the longest record}.  n_loci = 0 succeeds with
 * empty results.  Device memory is O(records + loci x samples), allocated and released by the call.  Nothing resident changes. */
int mirp_locus_scan(mirp_ctx* ctx, const MirpLocusSpan* loci, int64_t n_loci, const MirpLocusOpts* opts, MirpCluster** out, int64_t** sample_counts,
                    int64_t stats[5]);

/* siRNA duplexes and the 5' overlap signature on given loci on the context's resident alignments, all samples pooled (the sample
 * field is not looked at).  A record is kept when min_len <= len <= max_len; its 5' end is f = pos on '+' and pos + len - 1 on '-'; it belongs
 * to every locus [start, end] of its contig with start <= f <= end (5'-end membership, not mirp_locus_scan's span overlap; the locus strand is
 * ignored).  With U(x) / V(y) the depth sums of the kept '+' / '-' records whose 5' end is x / y, the signature of a locus is
 * H[k] = sum over x in [start, end] with x + k - 1 <= end of min(U(x), V(x + k - 1)), k = 1 .. max_overlap.  A duplex is a '+' placement
 * (p, L) and a '-' placement (p - overhang, L) of kept records (a placement = a distinct (pos, strand, len) with its depth sum) whose 5' ends p
 * and p - overhang + L - 1 both lie in the locus; its paired reads are m = min of the two sums. */
typedef struct {
    const int64_t* contig_len;      /* LN of contigs 0 .. n_contigs - 1, each 0 .. 2^31 - 1 */
    int32_t n_contigs, min_len, max_len, max_overlap, overhang, reserved;   /* 1 <= min_len <= max_len <= 65535; max_overlap 1 .. 64; overhang 0 .. 8, < min_len */
    int64_t min_reads;              /* a duplex with m >= min_reads (>= 1) is listed */
} MirpSignatureOpts;
/* Per locus: the depth sums of its member records (all, '+'), the number of duplexes and the sum of their m, and the major duplex (largest m;
 * ties to the smallest p, then the shorter L): p, the two depth sums and L; the five major fields are 0 for a locus without a duplex. */
typedef struct { int64_t reads, plus_reads, duplexes, duplex_reads, major_pos, major_plus, major_minus; int32_t major_len, reserved; } MirpSignatureRow;
/* One listed duplex: the locus (index in the call), p, the depth sums of the '+' and the '-' placement, L. */
typedef struct { int64_t locus, pos, plus_reads, minus_reads; int32_t len, reserved; } MirpDuplexSite;
/* Table rows (U entries, placements) one wave-job serves, and the largest max_overlap.  No result depends on where a chunk ends. */
#define MIRP_SIGNATURE_CHUNK 4096
#define MIRP_SIGNATURE_MAX_OVERLAP 64
/* Out: *rows holds one MirpSignatureRow per locus in input order; *overlaps H as n_loci x max_overlap, row-major (column k - 1 = overlap k);
 * *sites the *n_sites listed duplexes ordered by (locus, p, L), a duplex that lies in several loci once under each; each is released with
 * mirp_free.  stats (optional) = {records, kept records, U entries, V entries, (locus, chunk of U entries) jobs of the overlap kernel, duplex
 * sites written}; the entries of U and V are the distinct 5' ends that lie on their contig (1 .. LN), which are all a locus can hold; with
 * n_loci = 0 nothing runs on the device and stats[1 .. 5] are 0.  A bad argument (a null pointer, n_loci outside 0 .. 2^24, an option out of
 * its range, overhang >= min_len, a contig length outside 0 .. 2^31 - 1, a locus with a tid outside the table, start < 1, start > end or
 * end > LN) is refused with -1 before anything is allocated on the device.  n_loci = 0 succeeds with empty results.  Device memory is
 * O(records + loci x max_overlap + sites), allocated and released by the call.  Nothing resident changes. */
int mirp_signature_scan(mirp_ctx* ctx, const MirpLocusSpan* loci, int64_t n_loci, const MirpSignatureOpts* opts, MirpSignatureRow** rows,
                        int64_t** overlaps, MirpDuplexSite** sites, int64_t* n_sites, int64_t stats[6]);

/* Differential expression between two groups of samples: the exact negative-binomial test of Anders & Huber 2010 on a feature x
 * sample count matrix, as mirp_cluster_scan, mirp_isomir_scan and mirp_locus_scan write it.  counts: n_features x n_samples, row-major, the
 * used samples only.  The size factors, the common dispersion, the adjustment of the p-values and all text are the host's; the moments of
 * every feature and the whole test (one term per read of a feature) run on the device. */
typedef struct {
    const double* size_factor;      /* n_samples values, each finite and > 0 */
    const uint8_t* group;           /* n_samples values: 0 = group A, 1 = group B */
    int32_t n_samples;              /* 2 .. 255 */
    int32_t mode;                   /* dispersion: 0 max(raw, common), 1 common, 2 max(raw, 0) per feature, 3 `phi` for every feature */
    double phi;                     /* mode 3: the dispersion, >= 0 (0 = the Poisson case, an exact binomial test); otherwise ignored but checked */
    double min_mean;                /* the common dispersion is the median raw dispersion of the features with base_mean >= min_mean */
    double pseudo;                  /* log2fc = log2((mean_b + pseudo) / (mean_a + pseudo)) */
} MirpDiffexpOpts;
typedef struct {
    double base_mean, mean_a, mean_b, log2fc, dispersion, p;   /* p = -1: an untested feature (no read in the used samples) */
    uint64_t k_a, k_b;                                         /* raw counts of the two groups */
} MirpDiffexpRow;
/* Terms one wave-job of the test serves, the most features of a call and the bound of a count and of the terms of a call.  For tests of the
 * sizes around a multiple of the chunk: no result depends on where a chunk ends beyond the rounding of a sum. */
#define MIRP_DIFFEXP_CHUNK 4096
#define MIRP_DIFFEXP_MAX_FEATURES 16777216
#define MIRP_DIFFEXP_MAX_COUNT 1099511627776
/* With y = count / size factor: base_mean, mean_a, mean_b = the means of y over all used samples and over either group; the raw dispersion is
 * (v - z) / base_mean^2 (0 where base_mean = 0, or where no group has two samples), v the pooled within-group variance of y over the groups
 * with two or more samples, z = base_mean x the mean of 1 / size factor.  The common dispersion is max(0, the median raw dispersion over the
 * features with base_mean >= min_mean); without such a feature modes 0 and 1 fail with -10 (mode 2 reports 0).  `dispersion` is the value
 * the test used.  p is the two-sided exact test conditioned on n = k_a + k_b: the probability of every split (a, n - a) that is at most as
 * likely as the observed one (within the relative slack 1e-7), over that of all n + 1 splits; 0 where the latter overflows a double.
 * A bad argument (a null pointer, n_features outside 0 .. 2^24, n_samples outside 2 .. 255, a group value above 1, an empty group, a size
 * factor that is not finite and > 0, a negative or non-finite phi, min_mean or pseudo, a mode outside 0 .. 3, modes 0 .. 2 without a group
 * of two or more samples, a count >= 2^40, more than 2^40 terms = the sum of n + 1 over the features) is refused with -1 before anything is
 * allocated on the device.  Out: *rows (release with mirp_free) one MirpDiffexpRow per feature in input order; stats (optional) = {features,
 * features tested, (feature, chunk) jobs, terms, the bits of the common dispersion as a double (mode 3: of phi)}.  n_features = 0 succeeds
 * with an empty result.  Device memory is O(features x samples + jobs), allocated and released by the call.  Nothing resident changes.  Two
 * calls on the same input return the same bytes: every sum is made in a fixed order, without floating-point atomics. */
int mirp_diffexp(mirp_ctx* ctx, const uint64_t* counts, int64_t n_features, const MirpDiffexpOpts* opts, MirpDiffexpRow** rows, int64_t stats[5]);

/* isomiR counts: aligned reads, with or without the 3' tails of `align --tail`, joined against annotated miRNAs.
 *
 * The tailed tokenizer reads SAM files as mirp_tokenize_sams does (threads, no device; @SQ table of the first file, one sample per file, records
 * with flag & 0x704 dropped, depth N of the read id `_xN`, CRLF; the same refusals and messages) but keeps the templated footprint and the tail:
 * alns[k] = {tid, pos = POS, depth, len = m, strand, sample} and tails[k] = the tail code, in (sample, file) order.  CIGAR `<m>M`: no clip;
 * `<m>M<t>S` on +, `<t>S<m>M` on -: a 3' clip of t >= 1 bases whose letters as sequenced are the tail (SEQ[m:], or the reverse complement of
 * SEQ[:t]); without a clip the value of the first XT:Z: tag is the tail (`align --tail-trim`).  Letters: upper-cased, U = T, anything outside
 * ACGT = N.  Tail code: 0 = none, else (5^t - 5) / 4 + 1 + the digits A0 C1 G2 T3 N4 as a base-5 number, first letter first (1 .. 488,280; ordered
 * by length, then letters).  Any other CIGAR, m outside 1..65535, len(SEQ) != m + t, or a clip with SEQ `*` skips the record (skipped_cigar); a
 * tail of more than 8 letters skips it (skipped_long_tail).  Returns 0 or -1 with a message in errbuf; release with mirp_free_tailed_sam_data. */
typedef struct {
    int32_t n_contigs;  char* contig_names;   /* NUL-separated, @SQ order of the first file */
    int64_t* contig_len;
    int32_t n_samples;  char* sample_names;   /* NUL-separated, one per file */
    MirpAln* alns; uint32_t* tails; int64_t n_alns;
    int64_t skipped_cigar, skipped_long_tail;
} MirpTailedSamData;
int mirp_tokenize_sams_tailed(const char* const* paths, int32_t n_paths, int32_t n_threads, MirpTailedSamData* out, char* errbuf, size_t errbuf_len);
void mirp_free_tailed_sam_data(MirpTailedSamData* data);

/* One annotated miRNA: contig, strand (0 '+', 1 '-'), [start, end] 1-based inclusive.  Its number is its index in the array. */
typedef struct { int32_t tid, strand; int64_t start, end; } MirpIsoLocus;
typedef struct { int32_t max5, max3, n_samples, reserved; } MirpIsomirOpts;      /* max5, max3 0..15; n_samples 1..255 */
/* One isomiR: a distinct (locus, d5, d3, tail code) among the assigned records, with the 64-bit sum of their depths. */
typedef struct { int32_t locus, d5, d3; uint32_t tail; int64_t reads; } MirpIsomir;
/* Depth sums of one locus over its records: all, canonical (d5 = d3 = 0, no tail), d5 != 0, d3 < 0, d3 > 0, tailed, tail all T, tail all A; its
 * distinct isomiRs; the major isomiR (largest reads, ties to the first in isomiR order) as an index into the isomiR array, -1 without reads. */
typedef struct { int64_t reads, canonical, shift5, trim3, ext3, tailed, tail_u, tail_a, isomirs, major_reads, major; } MirpIsoLocusSum;
/* With r5 / r3 the 5' / 3' end of a record's footprint (pos and pos + len - 1 on +, swapped on -), l5 / l3 those of a locus and sigma = +1 / -1:
 * d5 = sigma (r5 - l5), d3 = sigma (r3 - l3), in 64-bit arithmetic.  A locus admits a record of its contig and strand with |d5| <= max5 and
 * |d3| <= max3; a record counts in the admitting locus with the smallest (|d5|, |d3|, locus number), or nowhere.  The records and tail codes are
 * the caller's (any order; nothing resident is read or changed), n_loci 1 .. 2^24, a counted record with sample >= n_samples is refused.
 * Out (each released with mirp_free): *isomirs holds the *n_isomirs isomiRs ordered by (locus, d5, d3, tail), d5 and d3 signed; sums[n_loci];
 * locus_counts[n_loci x n_samples] and isomir_counts[n_isomirs x n_samples], row-major depth sums; stats (optional) = {records, records
 * assigned, depth assigned, isomiRs}.  Device memory is O(records + loci x samples + isomiRs x samples), allocated and released by the call. */
int mirp_isomir_scan(mirp_ctx* ctx, const MirpAln* alns, const uint32_t* tails, int64_t n, const MirpIsoLocus* loci, int64_t n_loci,
                     const MirpIsomirOpts* opts, MirpIsomir** isomirs, int64_t* n_isomirs, MirpIsoLocusSum** sums, int64_t** locus_counts,
                     int64_t** isomir_counts, int64_t stats[4]);

/* Degradome (PARE / GMUCT) evidence of miRNA-guided cleavage on the context's resident alignments (after any SAM ingest, or after
 * mirp_load_alignments): the degradome reads aligned to the transcripts.  A sense record (plus strand, 1 <= pos <= LN) is a read of the unit (tid,
 * pos); a unit's abundance is the sum of its records' depths; its category 0..4 follows CleaveLand's (4: one read; 0: the transcript's only maximum;
 * 1: one of several maxima; 2: above the transcript's mean over occupied positions; 3: the rest).  Every miRNA is evaluated at every unit of category
 * <= max_category, only at the site whose position 10 pairs with the unit's position, with the score and the cleavage_site rule of mirp_target_scan;
 * a hit has half-score <= max_half_score and p <= alpha, p = 1 - (1 - c_k / P)^N with N = the miRNA's plus-strand sites in all transcripts at or
 * below the hit's score, c_k = the units of the hit's category or better, P = the transcripts' bases.  contig_names (n_contigs NUL-terminated
 * strings) and contig_len are the @SQ lines the records' tids index: each must be a transcript of the FASTA with that length. */
typedef struct {
    int32_t max_half_score, cleavage_site, max_category, n_contigs;
    double alpha;                   /* 0 < alpha <= 1 */
    const char* contig_names;
    const int64_t* contig_len;
} MirpDegradomeOpts;
/* Reads the miRNA FASTA and the transcript FASTA as mirp_target_scan does (same refusals) and writes the TSV of §18 to out_path: a header line, then
 * one line per hit ordered by miRNA (file order), category, score, transcript (FASTA order), cleavage position.  Further refusals (-10): an @SQ contig
 * that is not in the FASTA or has another length there.  On any error the file at out_path is removed.  Out: stats = {miRNAs, transcripts, bases,
 * records, sense records, minus-strand records, units, C_0 .. C_4, evaluations (kept units x miRNAs), hits written, passes}; seconds = {parse, upload,
 * units + categories, site counts, anchored counts, key passes + sort + write}.  Passes hold at most mirp_set_target_capacity keys.  Nothing
 * resident changes. */
int mirp_degradome_scan(mirp_ctx* ctx, const char* mirna_path, const char* transcripts_path, const MirpDegradomeOpts* opts, const char* out_path,
                        int64_t stats[15], double seconds[6]);

/* Annotation of miRNAs against known miRNAs: every query against every kept known sequence, same sense, ungapped.  At shift d
 * query position i lies on known position i + d; offset5 = d, offset3 = Lq + d - Lk, mismatches over the overlap (an unknown letter mismatches
 * everything); a shift is admissible when |offset5| <= max_offset (0..4), |offset3| <= max_offset and mismatches <= max_mismatches (0..6); a pair
 * with an admissible shift is a hit, reported at the shift that minimises (distance = mismatches + |offset5| + |offset3|, mismatches, |d|, d).
 * max_lines: the first N lines per query in output order (0 = all).  species: n_species NUL-terminated prefixes; with n_species > 0 only the known
 * sequences whose id starts with one of them followed by '-' are kept. */
typedef struct {
    int32_t max_offset, max_mismatches, n_species, reserved;
    int64_t max_lines;
    const char* species;
} MirpAnnotateOpts;
/* Reads the query FASTA as mirp_target_scan reads its miRNA FASTA (same refusals) and the known FASTA files known_paths[0 .. n_known) with the same
 * rules, except that a record of length outside 12..32 is skipped and counted and that the id is the first word of the header; at most 2^24 known
 * sequences are kept (-10 beyond).  Writes the hits TSV of §19 to out_path (a header line, then one line per hit ordered by query (file order),
 * distance, mismatches, known (file order)) and one line per query to summary_path.  On any error both files are removed.  Out: stats = {queries,
 * known kept, known skipped, pairs, evaluations (pairs x shifts with both offsets within max_offset), hits, identical, isomir, homolog, novel, lines
 * written, passes}, seconds = {parse, upload, counting scan, key scans, sort + cut, download + write}.  Passes hold at most
 * mirp_set_target_capacity keys.  Nothing resident changes. */
int mirp_annotate_scan(mirp_ctx* ctx, const char* query_path, const char* const* known_paths, int32_t n_known, const MirpAnnotateOpts* opts,
                       const char* out_path, const char* summary_path, int64_t stats[12], double seconds[6]);

/* Shuffle test of precursor MFEs (randfold): every sequence is shuffled n_shuffles times on the device, the sequence and its shuffles
 * are folded with the context's fold model (mirp_set_fold_model) and the MFEs are reduced on the device to one record per sequence.  Letters: A C G U
 * in either case, T = U, codes 0..3; every other letter is code 4 and goes to the fold as N.  dinucleotide = 0: Fisher-Yates over the letters; 1: the
 * Altschul-Erikson shuffle that keeps every dinucleotide count and both ends.  The random numbers are a stateless function of (seed, sequence index
 * in this call, shuffle index, draw number), §20.  capacity: sequences folded per pass (0 = the default, 262,144); no result depends on it. */
typedef struct {
    uint64_t seed;
    int32_t n_shuffles;   /* 1..100000 */
    int32_t dinucleotide; /* 0 mono, 1 di */
    int64_t capacity;     /* 0 = default */
} MirpRandfoldOpts;
/* len; gc = letters C and G; mfe of the sequence (0.01 kcal/mol, the global minimum: mirp_fold_batch's mfe at any span >= len); le = shuffles with
 * mfe <= the sequence's; min_mfe = the smallest shuffled mfe; sum / sum_sq = the sum of the shuffled mfes / of their squares. */
typedef struct {
    int32_t len, gc, mfe, le, min_mfe, reserved;
    int64_t sum, sum_sq;
} MirpRandfoldRec;
/* seqs / offsets as mirp_fold_batch.  Refused with -10 and the record (1-based) named in mirp_last_error: an empty sequence, a sequence longer than
 * 3,000 nt, a byte >= 0x80, n_seqs x (n_shuffles + 1) beyond 2^40.  Out: recs[n_seqs] (library-owned, mirp_free); stats = {sequences, folds, passes,
 * fold fallbacks}; seconds = {upload, shuffle, fold, statistics, download}.  Only the records come back: no shuffled sequence and no per-shuffle MFE
 * leaves the device.  Nothing resident changes. */
int mirp_randfold(mirp_ctx* ctx, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpRandfoldOpts* opts, MirpRandfoldRec** recs,
                  int64_t stats[4], double seconds[5]);
/* For tests: the shuffles k = k0 .. k0 + n_k - 1 (k0 >= 0, n_k >= 1, k0 + n_k <= 100000) of every sequence as ACGUN bytes, row-major, sequence q's
 * rows len(q) wide back to back (library-owned, mirp_free).  Same refusals as mirp_randfold. */
int mirp_shuffle_batch(mirp_ctx* ctx, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpRandfoldOpts* opts, int32_t k0, int32_t n_k,
                       char** out, int64_t* n_bytes);

/* Two-strand (intermolecular) minimum free energy fold: the RNAduplex recursion on the Turner-2004 tables with dangles = 2,
 * whatever mirp_set_fold_model says.  Strands a and b are both 5'->3'; A C G U in either case, T = U, every other byte N, which pairs with
 * nothing.  mfe in 0.01 kcal/mol, 0 = unbound (then pairs and the four bounds are 0); pairs = base pairs of the structure; a_first .. a_last and
 * b_first .. b_last = the 1-based ends of the paired stretch of either strand. */
typedef struct { int32_t mfe, pairs, a_first, a_last, b_first, b_last; } MirpDuplexRec;
/* Pair q = a_blob[a_off[q] .. a_off[q + 1]) with b_blob[b_off[q] .. b_off[q + 1]), q < n.  Every strand has 1..64 nt: another length is refused
 * with -10 and the 1-based pair in mirp_last_error; n < 0 is refused with -1; n = 0 is fine.  Out: recs[n]; structures (may be NULL): the text of
 * pair q -- a as ( and ., then &, then b as ) and . -- NUL-terminated, at the sum over the pairs before q of len a + len b + 2.  The pairs are
 * folded in passes of bounded device memory (mirp_set_duplex_capacity); no result depends on the split.  Nothing resident changes. */
int mirp_duplex_batch(mirp_ctx* ctx, const char* a_blob, const int64_t* a_off, const char* b_blob, const int64_t* b_off, int32_t n, MirpDuplexRec* recs,
                      char* structures);
/* Pairs one pass of mirp_duplex_batch holds on the device; 0 = the default, 2^20.  Lowered only to test the split. */
int mirp_set_duplex_capacity(mirp_ctx* ctx, int64_t pairs);
/* stats = {pairs, passes, loop evaluations (predecessor cells read)} of the last mirp_duplex_batch. */
int mirp_duplex_last_stats(mirp_ctx* ctx, int64_t stats[3]);

/* Partition function of whole sequences (McCaskill inside / outside fold): Turner-2004 with dangles = 2, whatever
 * mirp_set_fold_model says.  Letters as mirp_duplex_batch.  bpp_cutoff: with want_bpp the pairs with p >= bpp_cutoff come back (0 <= cutoff <= 1). */
typedef struct {
    double bpp_cutoff;
    int32_t want_bpp;
    int32_t reserved;
} MirpEnsembleOpts;
/* len; mfe = the global minimum free energy (0.01 kcal/mol; mirp_fold_batch's mfe with the default model); efe = -kT ln Z (kcal/mol); mfe_freq =
 * exp(-(mfe / 100 - efe) / kT); diversity = 2 sum p (1 - p), the mean pair distance of the ensemble; the centroid holds the centroid_pairs pairs
 * with p > 0.5; centroid_dist = its mean pair distance to the ensemble. */
typedef struct {
    int32_t len, mfe;
    double efe, mfe_freq, diversity, centroid_dist;
    int32_t centroid_pairs, reserved;
} MirpEnsembleRec;
/* one pair of sequence `seq` (0-based index in the call), 1-based positions i < j */
typedef struct {
    int32_t seq, i, j, reserved;
    double p;
} MirpBpp;
/* seqs / offsets as mirp_randfold, with its refusals (-10 and the 1-based record in mirp_last_error: an empty sequence, one longer than 3,000 nt, a
 * byte >= 0x80); n_seqs = 0 is fine.  Out: recs[n_seqs] (caller's); centroids (caller's, the sum of len + 1 bytes): the dot-bracket texts,
 * NUL-terminated, back to back; with opts->want_bpp, *bpp (library-owned, mirp_free) holds the *n_bpp pairs with p >= bpp_cutoff ordered by
 * (seq, i, j) -- bpp and n_bpp may be NULL otherwise.  The sequences are folded in passes whose slabs fit mirp_set_ensemble_capacity; a
 * sequence's results are bit-identical whatever else is in the call and however it is split.  Nothing resident changes. */
int mirp_ensemble(mirp_ctx* ctx, const char* seqs, const int64_t* offsets, int32_t n_seqs, const MirpEnsembleOpts* opts, MirpEnsembleRec* recs,
                  char* centroids, MirpBpp** bpp, int64_t* n_bpp);
/* Bytes of table slabs one pass of mirp_ensemble holds on the device; 0 = the default, 2^35.  A sequence whose slab alone is larger runs in a
 * pass of its own.  Lowered only to test the split. */
int mirp_set_ensemble_capacity(mirp_ctx* ctx, int64_t bytes);
/* stats = {sequences, passes, cells (i < j pairs of positions, summed over the sequences)} of the last mirp_ensemble. */
int mirp_ensemble_last_stats(mirp_ctx* ctx, int64_t stats[3]);

/* Accessibility of an interval: with the model of mirp_ensemble, efe = -kT ln Z over all structures of the sequence, efe_open =
 * -kT ln Z_open over those in which no position of the interval is paired (pairs that enclose it are allowed), and upe = efe_open - efe >= 0 =
 * -kT ln P(the interval is unpaired), all in kcal/mol. */
typedef struct { double efe, efe_open, upe; } MirpUnpairedRec;
/* Window q = blob[off[q] .. off[q + 1]) with the 1-based interval lo[q] .. hi[q], q < n; letters as mirp_duplex_batch.  Refusals (-10 and the
 * 1-based record in mirp_last_error): an empty sequence, one longer than 128 nt, a byte >= 0x80, an interval outside 1 <= lo <= hi <= length;
 * n < 0 is refused with -1; n = 0 is fine.  Out: recs[n].  The windows are folded in passes of at most mirp_set_unpaired_capacity windows; a
 * window's record is bit-identical whatever else is in the call and however it is split.  Nothing resident changes. */
int mirp_unpaired_batch(mirp_ctx* ctx, const char* blob, const int64_t* off, const int32_t* lo, const int32_t* hi, int32_t n, MirpUnpairedRec* recs);
/* Windows one pass of mirp_unpaired_batch holds on the device; 0 = the default, 2^20.  Lowered only to test the split. */
int mirp_set_unpaired_capacity(mirp_ctx* ctx, int64_t windows);
/* stats = {windows, passes, cells (i < j pairs of positions, summed over the windows)} of the last mirp_unpaired_batch. */
int mirp_unpaired_last_stats(mirp_ctx* ctx, int64_t stats[3]);
/* The longest window whose tables mirp_unpaired_batch keeps in LDS; a longer one has them in device memory.  A constant of the build, for tests
 * of the lengths around it: no result depends on where the tables lie. */
int mirp_unpaired_lds_longest(void);
/* The flanks of the windows of mirp_target_scan's accessibility column: `up` bases towards the 5' end of the target strand and `down` towards
 * its 3' end (defaults 17 and 13).  Each >= 0, up + down <= 95 (a window never exceeds 33 + 95 = 128 nt); anything else is refused with -1. */
int mirp_set_target_flanks(mirp_ctx* ctx, int32_t up, int32_t down);

/* Gapped local alignment of query sequences (predicted precursors) with known sequences (miRBase hairpins), same sense: Gotoh's
 * recurrences with +match / -mismatch per column and gap_open + g * gap_extend per gap of g bases; letters A C G U/T in either case, anything
 * else mismatches everything.  match, mismatch 1..10, gap_open 0..20, gap_extend 1..10, min_score >= 1, max_lines >= 0 (0 = all). */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend, min_score, reserved;
    int64_t max_lines;
} MirpHairpinOpts;
/* One hit: 0-based indices of the query and the known sequence in the call, the score, the aligned spans (1-based, inclusive) and the counts of
 * the alignment's columns: `=`, `X`, runs of `I` or `D`, and `I` + `D` columns. */
typedef struct {
    int32_t query, known, score, q_start, q_end, k_start, k_end, matches, mismatches, gap_opens, gap_bases, reserved;
} MirpHairpinHit;
/* Rows of the query a lane of the scoring kernel holds in registers (a strip); for tests of the lengths around it. */
#define MIRP_HAIRPIN_STRIP 16
/* q_blob / q_off and k_blob / k_off as mirp_ensemble's seqs / offsets, every length 1..3000.  Refusals (-10 and the side and the 1-based record in
 * mirp_last_error): an empty sequence, one longer than 3,000 nt, a byte >= 0x80, more than 2^24 known sequences; n_q = 0 or n_k = 0 is fine.
 * Out (library-owned, mirp_free; NULL when there is no hit): *hits holds the *n_hits pairs with score >= min_score ordered by (query, score
 * descending, known), at most max_lines per query; *ops one byte (`=` `X` `I` `D`; the query plays the read) per alignment column of every hit
 * in forward order, hit h at (*ops)[(*ops_off)[h] .. (*ops_off)[h + 1]).  A pair's hit and ops are the same bytes whatever else is in the call
 * and however it is split into passes.  Nothing resident changes. */
int mirp_hairpin_align(mirp_ctx* ctx, const char* q_blob, const int64_t* q_off, int32_t n_q, const char* k_blob, const int64_t* k_off, int32_t n_k,
                       const MirpHairpinOpts* opts, MirpHairpinHit** hits, int64_t* n_hits, char** ops, int64_t** ops_off);
/* Device bytes one pass of mirp_hairpin_align holds: the scoring stage's result buffer (8 bytes per pair; passes over ranges of queries) and the
 * traceback stage's direction matrices (1 byte per cell of q_end x k_end; passes over ranges of hits).  0 = the default, 2^31.  A query or a hit
 * that alone is larger runs in a pass of its own.  Lowered only to test the split. */
int mirp_set_hairpin_capacity(mirp_ctx* ctx, int64_t bytes);
/* stats = {queries, known, pairs, cells (query length x known length, summed over the pairs), hits (before the max_lines cut), passes (scoring +
 * traceback), scoring passes, traceback passes} of the last mirp_hairpin_align; seconds = {upload, scoring, filter + sort + cut, traceback,
 * download}.  hits_per_query (optional, n_q entries of the last call): the hits of every query before the cut. */
int mirp_hairpin_last_stats(mirp_ctx* ctx, int64_t stats[8], double seconds[5], int64_t* hits_per_query);

/* Homologs of known mature miRNAs in the genome of mirp_align_index: every placement of a known sequence within max_mismatches
 * (0..3) substitutions on either strand, all strata; the window of precursor_len (60..3000) around it, folded with span precursor_len; the
 * structure rules of the predict stage (a8, a9) on the placement's interval, without reads.  A query with more than max_placements (>= 1)
 * placements yields none.  `reserved` must be 0. */
typedef struct { int32_t max_mismatches, precursor_len, max_placements, reserved; } MirpHomologOpts;
/* One locus: the naming query (0-based index in the call) and its mismatches, the contig (index in reference order) and strand (0 '+', 1 '-'), the
 * mature, star, fold region and window as 1-based contig coordinates with exclusive ends, prime5 (1: the mature lies in the 5' arm), the base
 * pairs of the mature side of the duplex and the unpaired bases of both sides, the energy (0.01 kcal/mol) and length of the structure line the
 * structure comes from (normalised energy = energy / 100 / line_len), the structure's length, and n_also further placements at the same interval. */
typedef struct {
    int32_t query, contig, strand, mismatches;
    int32_t mat_s, mat_e, star_s, star_e, fold_s, fold_e, win_s, win_e;
    int32_t prime5, total_bps, total_dots, energy, line_len, ss_len, n_also, reserved;
    int64_t text_off, also_off;
} MirpHomologRec;
/* q_blob / q_off as mirp_hairpin_align's: n_q distinct known sequences of 18..26 letters A C G T/U in either case (anything else is refused with
 * -10 and the 1-based record in mirp_last_error).  Called after mirp_align_index; nothing of the index changes.  Out (library-owned, mirp_free;
 * NULL when there is no locus): *recs holds the *n_recs loci ordered by (contig, fold_s, strand, mat_s, mat_e); *text holds for record r at
 * text_off the win_e - win_s letters (A C G T N) of its window on its strand, followed by the ss_len characters of its dot-bracket structure,
 * which covers [fold_s, fold_e); *also holds n_also pairs (query, mismatches) per record from pair also_off on, in query order.  The result is the
 * same however the placements are split into passes and chunks. */
int mirp_homolog_scan(mirp_ctx* ctx, const char* q_blob, const int64_t* q_off, int32_t n_q, const MirpHomologOpts* opts, MirpHomologRec** recs,
                      int64_t* n_recs, char** text, int32_t** also);
/* The contigs of the resident index in reference order, which MirpHomologRec.contig indexes (library-owned, mirp_free): *names holds the
 * *n_contigs names, each followed by a NUL, *names_bytes bytes in all; *lens their lengths. */
int mirp_homolog_contigs(mirp_ctx* ctx, char** names, int64_t* names_bytes, int64_t** lens, int32_t* n_contigs);
/* Placement keys one scan pass holds on the device (0 = the default, 2^24; at least 1), placements per chunk of windows that is folded and evaluated
 * at once (0 = as many as 1 GiB of fold output holds, at most 32,768), structure lines the fold keeps per window at first (0 = 96), and the
 * evaluation kernel's first capacities: pieces per line, structures and staged lines per window (0 = the defaults; all three or none).  Lowered only
 * to test the multi-pass, multi-chunk and re-run paths. */
int mirp_set_homolog_capacity(mirp_ctx* ctx, int64_t keys, int64_t chunk, int32_t fold_lines, int32_t pieces, int32_t structures, int32_t staged_lines);
/* stats = {queries, queries dropped by max_placements, placements (= windows folded), placements with a passing structure, loci, scan passes,
 * chunks, folds (a chunk is folded again when a window needs more structure lines), evaluation re-runs, at 9 the launches of the evaluation kernel
 * whose staged structure text lay in global memory instead of LDS, 0 at 10, then at 10 + k the placements without a passing structure whose
 * structure of lowest normalised energy has get_maturestar_info code k = 1..12, and at 23 those whose structure list is empty} of the last
 * mirp_homolog_scan; seconds = {scan, windows, fold, evaluation + download, merge}. */
int mirp_homolog_last_stats(mirp_ctx* ctx, int64_t stats[24], double seconds[5]);

/* Inverted repeats of a genome: the banded local alignment of every contig with its own reverse complement.  Cell (i, j), i < j,
 * pairs base i with base j (A.T and C.G only; every other letter pairs with nothing); H(i, j) = max(0, H(i+1, j-1) +match / -mismatch,
 * H(i+1, j) - gap, H(i, j-1) - gap) over the cells with j - i + 1 <= max_span.  max_span 8..4096, min_score >= 1, match and mismatch 1..10,
 * gap 1..50; `reserved` must be 0. */
typedef struct { int32_t max_span, min_score, match, mismatch, gap, reserved; } MirpInvertedOpts;
/* One repeat: the 0-based contig of the call, the score, the two arms (1-based, inclusive; left_start < left_end + 1 <= right_start <= right_end)
 * and the counts of the alignment's columns: `=`, `X`, and `L` + `R` (a base of the left / right arm that pairs with nothing). */
typedef struct {
    int32_t contig, score;
    int64_t left_start, left_end, right_start, right_end;
    int32_t matches, mismatches, gaps, reserved;
} MirpInvertedRec;
/* Rows (left-arm positions) a wave of the row scan owns, rows of one strip (what its 64 lanes hold in registers at once; the rows beyond a tile
 * that a wave recomputes are ceil((max_span - 1) / strip) strips), and the largest max_span.  For tests of the lengths around them: no result
 * depends on where a tile or a strip ends. */
#define MIRP_INVERTED_TILE 8192
#define MIRP_INVERTED_STRIP 1024
#define MIRP_INVERTED_MAX_SPAN 4096
/* blob / off as mirp_ensemble's seqs / offsets: n_contigs contigs of any length (an empty one has no repeat).  Refusal (-10 and the 1-based contig
 * in mirp_last_error): a byte >= 0x80.  Out (library-owned, mirp_free; NULL when there is no repeat): *recs holds the *n_recs accepted repeats
 * ordered by (contig, left_start, right_end); *ops one byte (`=` `X` `L` `R`) per alignment column in outer-to-inner order, repeat r at
 * (*ops)[(*ops_off)[r] .. (*ops_off)[r + 1]).  A contig's repeats are the same whatever else is in the call and however the work is split into
 * passes.  Nothing resident changes. */
int mirp_inverted_scan(mirp_ctx* ctx, const char* blob, const int64_t* off, int32_t n_contigs, const MirpInvertedOpts* opts, MirpInvertedRec** recs,
                       int64_t* n_recs, char** ops, int64_t** ops_off);
/* Device bytes one pass of mirp_inverted_scan holds: a traceback pass's direction bytes (span x span per candidate) and a scan pass's row keys
 * (4 bytes per row, whole tiles).  0 = the default, 2^31.  A candidate or a tile that alone is larger runs in a pass of its own.  Lowered only
 * to test the splits. */
int mirp_set_inverted_capacity(mirp_ctx* ctx, int64_t bytes);
/* stats = {contigs, bases, cells of the band, rows with r >= min_score, candidates, candidates traced, candidates dropped without a traceback,
 * accepted repeats, scan passes, traceback passes, tiles, 0} of the last mirp_inverted_scan; seconds = {upload, scan, candidates + sort,
 * traceback + selection, download}. */
int mirp_inverted_last_stats(mirp_ctx* ctx, int64_t stats[12], double seconds[5]);

/* Natural antisense transcripts: pairs of transcripts a < b that are complementary over a long stretch, found by seed, join and
 * banded extension.  Cell (i, j) compares base i of A with base j of B', the reverse complement of B (Watson-Crick only; every letter but
 * A C G T/U equals nothing).  A seed hit is an exact k-mer of A and B' without such a letter, of a k-mer value that occurs at most max_occ times
 * in either sense; hits are binned by their shifted diagonal e = x - y + len(B) - 1 into bins of `band` diagonals, a bin with min_seeds hits is a
 * candidate, and H(i, j) = max(0, H(i-1, j-1) +match / -mismatch, H(i-1, j) - gap, H(i, j-1) - gap) runs over the bin and its two neighbours.
 * seed 12..24, band one of 16 32 64 128 256, max_occ 1..10000, min_seeds >= 1, match and mismatch 1..10, gap 1..50, min_score and min_length
 * >= 1; `reserved` must be 0. */
typedef struct { int32_t seed, band, max_occ, min_seeds, match, mismatch, gap, min_score, min_length, reserved; } MirpNatsOpts;
/* One region: the 0-based transcripts a < b of the call, the score, the interval of A and of B (1-based, inclusive, each in its own forward
 * coordinates) with the transcripts' lengths, the counts of the alignment's columns (`=`, `X`, and `I` + `D`: a base of A / of B without an
 * opposite base), the seed hits of the candidate it came from and that candidate's bin. */
typedef struct {
    int32_t a, b, score, a_start, a_end, a_len, b_start, b_end, b_len, matches, mismatches, gaps, seeds, bin;
} MirpNatsRec;
/* The longest transcript that is searched; a longer one (and an empty one) is skipped and counted, and keeps its index. */
#define MIRP_NATS_MAX_LEN 65535
/* blob / off as mirp_inverted_scan's: n_seqs transcripts.  Refusals (-10 and the 1-based transcript in mirp_last_error): a byte >= 0x80; more
 * than 2^25 transcripts.  Out (library-owned, mirp_free; NULL when there is no region): *recs holds the *n_recs regions ordered by (a, b,
 * a_start, b_start); *ops one byte (`=` `X` `I` `D`) per alignment column in A's 5'->3' order, region r at (*ops)[(*ops_off)[r] ..
 * (*ops_off)[r + 1]).  The regions are the same however the work is split into passes.  Nothing resident changes. */
int mirp_nats_scan(mirp_ctx* ctx, const char* blob, const int64_t* off, int32_t n_seqs, const MirpNatsOpts* opts, MirpNatsRec** recs, int64_t* n_recs,
                   char** ops, int64_t** ops_off);
/* Device bytes one pass of mirp_nats_scan holds: a join pass's seed hits (16 bytes each: the key and the sort's second buffer; whole transcripts
 * a) and a traceback pass's direction bytes.  0 = the default, 2^31.  A transcript or a candidate that alone is larger runs in a pass of its
 * own.  Lowered only to test the splits. */
int mirp_set_nats_capacity(mirp_ctx* ctx, int64_t bytes);
/* stats = {transcripts, skipped transcripts, bases, k-mer values ignored, seed hits, candidates, kept candidates, band cells of the kept
 * candidates, candidates with score >= min_score, candidates traced, regions, pairs, join passes, scan launches, traceback passes, 0} of the
 * last mirp_nats_scan; seconds = {upload + keys, sort + runs, join + candidates, band scan, traceback, selection}. */
int mirp_nats_last_stats(mirp_ctx* ctx, int64_t stats[16], double seconds[6]);

/* How many jobs a resident slot served, for the kernels whose workgroups (or waves) keep a private slab and serve several jobs in turn.  family:
 * 0 = the two-strand fold (a wave; mirp_duplex_batch, mirp_target_scan with energy), 1 = the accessibility kernel (a workgroup;
 * mirp_unpaired_batch, mirp_target_scan with accessibility), 2 = the scoring kernel of mirp_hairpin_align (queries per workgroup row), 3 = the
 * evaluation kernel of mirp_homolog_scan (a workgroup), 4 = the filter kernel (a workgroup serves windows it, it + grid, ...; mirp_predict_batch,
 * mirp_predict_batch_reasons, mirp_predict, mirp_predict_reasons; re-runs of windows over a capacity count as launches), 5 = the count kernel of mirp_locus_scan (a wave serves (locus, chunk) jobs w, w + waves, ...), 6 = the sum kernel of mirp_diffexp (a wave serves (feature, chunk) jobs w, w + waves, ...), 7 = the overlap kernel of mirp_signature_scan (a wave serves (locus, chunk of U entries) jobs w, w + waves, ...), 8 = the band scan of mirp_nats_scan (a wave serves candidates w, w + waves, ...).  out = {launches of that kernel, the largest ceil(jobs / slots) over them} of the last
 * of the named calls; each of them resets its families when it starts.  A record for tests: nothing reads it.  Another family is refused (-1). */
int mirp_last_jobs_per_slot(mirp_ctx* ctx, int32_t family, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif

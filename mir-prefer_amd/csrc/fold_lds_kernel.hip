// LDS-resident batched L-bounded Zuker local fold for precursor windows (n <= 350, span <= 300):
// the production case PRECURSOR_LEN = 300 (/root/reference/miR_PREFeR.py:90, RNALfold -L at :3053).
//
// One window per workgroup.  The geometry described here is the one of the dense pass and of the vienna-1.8.5 model -- 1024 threads = 16 wavefronts, one
// workgroup per CU; the default model's candidate-pool pass, which folds the product's windows, runs two 512-thread workgroups per CU without the
// fML triangle in LDS (see NT = LNT2 at the kernel):
//   * fML lives entirely in LDS as a triangular biased-uint16 table, diagonal-major: (d,i) -> off(d)+i, so
//     the two operands of a multiloop split are read at consecutive addresses by consecutive lanes;
//   * c keeps its last 32 anti-diagonals in an LDS ring (interior loops reach back MAXLOOP+2) and is
//     archived once, coalesced, as int16 to a per-window global slab for the exterior (f3) sweep
//     and the backtracks (fold_lds_epilogue_kernel);
//   * per anti-diagonal, phase A1 = interior-loop candidates with LANE = PAIRED CELL and WAVE = CANDIDATE GROUP:
//     every wave walks its own fixed share of the 496 (n1, n2) shapes for up to 64 paired cells at once, so the
//     loop shape is wave-uniform -- ring rows are scalar offsets, candidates are immediate offsets, size penalties
//     are scalar loads -- and one candidate costs one LDS read + add + min (generic shapes, ring stores
//     G0 = c + inner mismatch) or three LDS reads + four VALU ops (bulges and 1xn loops, through combined
//     per-window pair-code arrays).  Waves 0-7: generic rows (47 shapes each), 8-13: bulges / 1xn (18-19 each),
//     14: stack, 1-bulges, 2x3, 15: the 1x1/1x2/2x2 loops that read the big tables from global memory;
//   * phase A2 = multiloop splits (lane = cell, wave-uniform split point, scalar offsets); phase B = one thread per
//     cell finalises c, fML, DML, builds the ordered paired-cell list of diagonal d+2 (ballot compaction) and runs
//     in the same barrier interval as phase A of the next diagonal;
//   * INF needs no predicates: tables are biased unsigned 16-bit with INF = 65535, so any sum that involves
//     INF is >= 65535 and can never beat the 65535 start value of a running minimum;
//   * windows whose energies leave the 16-bit ranges are flagged and re-run by the generic kernel.
// No MFMA: integer min-plus DP with irregular table lookups.
#include <algorithm>
#include "fold_lds_common.h"
#include "fold_ctl.h"      // the control block's words, named once for fold_lds_kernel_body.h and the driver
// In-place compaction of the split-candidate pool, period in diagonals per model (0 = never) and the number of 64-entry rounds a wave holds in registers.
#ifndef MIRP_CPERIOD0
#define MIRP_CPERIOD0 0       // default model: never (925 entries: a compaction's two barriers cost more than the dead lanes; measured 60.9 / 61.7 / 62.1 / 62.9 ms at never / 128 / 64 / 32)
#endif
#ifndef MIRP_CPERIOD1
#define MIRP_CPERIOD1 64      // vienna-1.8.5 (1,283 pair entries, 70 instructions per visit): 89.5 ms without, 87.3 / 85.9 / 85.6 / 85.0 at 8 / 16 / 32 / 64
#endif
#define CPOOL_ROUNDS 4
#ifndef MIRP_A1_FUSE
#define MIRP_A1_FUSE 1        // default model, two windows per CU: both roles of a wave in one pass over the blocks (0: timing build, role-outer as before round 12)
#endif
#ifndef MIRP_PHASEB_SKIP
#define MIRP_PHASEB_SKIP 1    // default model, two windows per CU: waves without a cell of the diagonal branch round phase B (0: timing build, see phaseB0)
#endif
#ifndef MIRP_RAMP_MIX
#define MIRP_RAMP_MIX 1       // default model, two windows per CU: lanes go ahead on the first interior-loop diagonals as well (0: timing build, see `mix` in the body)
#endif

namespace mirp {

// MODEL 0: vienna-2.1.2 (Turner-2004, dangles 2).  MODEL 1: vienna-1.8.5 (Turner-1999 values in the same parameter layout, dangles 1: four-way
// dangle minima in the multiloop closing and the fML pair terms, fML also on the diagonal d = span; SURVEY.md Appendix B, d1 column).
//
// SPARSE (the product's first pass): the multiloop splits DML(i,j) = min_s fML(i,s-1) + fML(s,j) run over split CANDIDATES only.  With ML_BASE = 0
//     DML(i,j) = min( DML(i,j-1),  min over s in Cand(j), i+TURN+2 <= s <= j-TURN-1, of fML(i,s-1) + fML(s,j) ),
// Cand(j) = { s : fML(s,j) is realised STRICTLY by its pair term c(s,j) + MLstem } -- an entry that equals fML(s+1,j) is dominated by the split at
// s+1 (fML(i,s) <= fML(i,s-1)), one that equals fML(s,j-1) is a split of (i,j-1), one that equals DML(s,j) = fML(s,u-1) + fML(u,j) is dominated by
// the split at u.  The tables stay bit-identical (tests/tools/splitcand_gate.c checks the identity cell by cell on the CPU oracle's tables and
// counts: 925 candidates per benchmark window, 2.5 % of the dense loop's relaxations).  Phase B appends the candidates it finds to a pool
// {s-1, j, fML(s,j)} behind the window's fML triangle; phase A2 maps LANE = POOL ENTRY: the entry's column j holds exactly one cell of the
// diagonal at hand, (j-d, j), which it relaxes with one gather + one LDS atomic minimum.  A row's thread carries DML(i,j-1) in a register.
// A window whose pool overflows (tandem repeats) or whose length leaves no room for one is handed to the dense instantiation (second launch).
//
// NT = LNT2 (the product's first pass of the default model): TWO windows per CU, each on a 512-thread workgroup with half of the LDS.  The fML
// triangle -- 103 of the 160 KB at n = 325 -- is not kept in LDS: phase B holds the last two diagonals in a ring (all it reads itself) and stores every
// cell to the window's archive slab in the tiled layout the epilogue reads (so no copy-out pass at the end of a window either); the sparse splits
// take their one operand per pool entry and diagonal, fML(i, s-1), from that slab.  An entry reads the table at a fixed lag behind the wavefront
// (the length of its right operand, at least 5 diagonals), so its address is known ahead: the gather is issued before the interior loops of the
// interval and consumed behind them.
// Visibility of those cells: producer and consumer are waves of ONE workgroup, i.e. of one CU and one vector L1, and the cell a gather of
// interval d reads was stored by phase B at least three __syncthreads() earlier.  __syncthreads() is a workgroup-scope release / acquire fence
// over global memory as well.  What that fence compiles to here is s_waitcnt lgkmcnt(0) alone in front of every s_barrier -- NOT a drain of the
// stores: the only vmcnt(0) of an interval stands at the top of phase B.  That is the compiler's workgroup-scope rule for a kernel that does not
// run in threadgroup-split mode (this one does not): all waves of the workgroup sit on one CU, their vector memory operations go through that
// CU's one L1 in the order they were issued, and stores write through it, so a store issued before the producer's barrier is ahead, in that L1,
// of any load a consumer issues behind the barrier.  Only tgsplit code objects need vmcnt(0) for workgroup scope.  Nothing is handed between
// workgroups.  Plain loads are therefore enough -- no sc1, no cache invalidate -- and nothing here relies on timing.
// The 16 interior-loop roles run two to a wave (see `role` in phase A1).  The two workgroups of a CU have independent barrier chains: one window's barrier wait
// and phase-B chain are covered by the other window's interior loops.
template <int MODEL, bool SPARSE, int NT = LNT>
__global__ void __launch_bounds__(NT, 4) fold_lds_kernel(
    const FoldParams* __restrict__ P, const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ win_lens,
    int n_work, int win_base, int span, short* __restrict__ slabs, size_t slab_shorts, int* __restrict__ win_state,
    unsigned int* __restrict__ work_counter, int* __restrict__ fallback_list,
    unsigned int* __restrict__ fallback_count, int max_lines, int ss_stride, MirpFoldLine* __restrict__ out_lines, char* __restrict__ out_ss,
    int* __restrict__ out_nlines, int* __restrict__ out_mfe, int* __restrict__ out_status, int light_clocks_arg, long long* __restrict__ dbg_cycles_arg,
    const int* __restrict__ todo_list, const unsigned int* __restrict__ todo_count, int* __restrict__ dense_list, unsigned int* __restrict__ dense_count) {
#include "fold_lds_kernel_body.h"
}

// The candidate-pool pass of the default model (two windows per CU) shares its CUs with epilogue workgroups (fold overlap, mirp_run_fold): its
// registers are capped so that four of its waves leave a SIMD the 64 registers of one epilogue wave.  amdgpu_num_vgpr counts in pairs on gfx950
// (unified register file): 56 -> at most 112 VGPRs; the kernel takes 111, none spilled, no scratch (120 without the cap).  96 VGPRs -- room for two
// epilogue waves -- cost 3 spilled registers and 16 bytes of scratch per lane.  The attribute takes no template argument, hence an explicit
// specialization, with the same body.
template <int MODEL, bool SPARSE, int NT>
__device__ __forceinline__ void fold_lds_body(

    const FoldParams* __restrict__ P, const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ win_lens,
    int n_work, int win_base, int span, short* __restrict__ slabs, size_t slab_shorts, int* __restrict__ win_state,
    unsigned int* __restrict__ work_counter, int* __restrict__ fallback_list,
    unsigned int* __restrict__ fallback_count, int max_lines, int ss_stride, MirpFoldLine* __restrict__ out_lines, char* __restrict__ out_ss,
    int* __restrict__ out_nlines, int* __restrict__ out_mfe, int* __restrict__ out_status, int light_clocks_arg, long long* __restrict__ dbg_cycles_arg,
    const int* __restrict__ todo_list, const unsigned int* __restrict__ todo_count, int* __restrict__ dense_list, unsigned int* __restrict__ dense_count) {
#if MIRP_A1_FUSE
#define MIRP_A1_FUSED      // this copy of the body is the two-windows-per-CU instantiation alone: its interior loops run block-outer (see MIRP_A1_FUSED there)
#endif
#include "fold_lds_kernel_body.h"
#undef MIRP_A1_FUSED
}
#ifndef MIRP_FILL_TWO_ATTR
#define MIRP_FILL_TWO_ATTR __attribute__((amdgpu_num_vgpr(56)))
#endif
template <>
__global__ void MIRP_FILL_TWO_ATTR __launch_bounds__(LNT2, 4) fold_lds_kernel<0, true, LNT2>(

    const FoldParams* __restrict__ P, const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ win_lens,
    int n_work, int win_base, int span, short* __restrict__ slabs, size_t slab_shorts, int* __restrict__ win_state,
    unsigned int* __restrict__ work_counter, int* __restrict__ fallback_list,
    unsigned int* __restrict__ fallback_count, int max_lines, int ss_stride, MirpFoldLine* __restrict__ out_lines, char* __restrict__ out_ss,
    int* __restrict__ out_nlines, int* __restrict__ out_mfe, int* __restrict__ out_status, int light_clocks_arg, long long* __restrict__ dbg_cycles_arg,
    const int* __restrict__ todo_list, const unsigned int* __restrict__ todo_count, int* __restrict__ dense_list, unsigned int* __restrict__ dense_count) {
    fold_lds_body<0, true, LNT2>(P, seqs, offs, win_lens, n_work, win_base, span, slabs, slab_shorts, win_state, work_counter, fallback_list, fallback_count, max_lines, ss_stride, out_lines, out_ss, out_nlines, out_mfe, out_status, light_clocks_arg, dbg_cycles_arg, todo_list, todo_count, dense_list, dense_count);
}

// ------------------------------------------------------------------------------------------
// Epilogue kernel: exterior sweep, enumeration, backtracks, output.  Latency-bound pointer chasing with global
// (L2) table reads, so it runs as many small workgroups (256 threads, ~16 KB LDS) per CU instead of sharing the
// fill kernel's one-workgroup-per-CU geometry.
// ------------------------------------------------------------------------------------------
#ifndef ENT
#define ENT 256
#endif
#ifndef MIRP_EPI_WGS
#define MIRP_EPI_WGS 8
#endif
__global__ void __launch_bounds__(ENT, MIRP_EPI_WGS) fold_lds_epilogue_kernel(
    const FoldParams* __restrict__ P, const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ win_lens,
    int n_work, int span, const short* __restrict__ slabs, size_t slab_shorts, const int* __restrict__ win_state, unsigned int* __restrict__ work_counter,
    int max_lines, int ss_stride, MirpFoldLine* __restrict__ out_lines, char* __restrict__ out_ss, int* __restrict__ out_nlines,
    int* __restrict__ out_mfe, int* __restrict__ out_status) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nc = LCAP + 8;
    int* f3 = (int*)smem;                                            // nc
    int* starts = f3 + nc;                                           // max_lines
    int* lens = starts + max_lines;                                  // max_lines
    int* btstk = lens + max_lines;                                   // (ENT/64)*3*BT_STACK
    int* misc = btstk + (ENT / 64) * 3 * BT_STACK;                   // 16
    int* off = misc + 16;                                            // LDMAX + 2
    short* spec = (short*)(off + LDMAX + 2);                         // 3*nc
    unsigned char* S = (unsigned char*)(spec + 3 * nc);              // nc
    unsigned char* seq = S + nc;                                     // nc
    char* btbuf = (char*)(seq + nc);                                 // (ENT/64)*nc
    EpiTables* EP = (EpiTables*)(smem + ((((size_t)(btbuf - (char*)smem) + (ENT / 64) * nc) + 15) & ~(size_t)15));
    short* xtab = (short*)(EP + 1);                                  // XTAB_N
    unsigned char* pq2 = (unsigned char*)(xtab + XTAB_N);            // nc
    short* ppart = (short*)(pq2 + nc);                               // nc
    const int tid = threadIdx.x;
    fill_epi_tables(EP, P, tid, ENT);
    fill_ext_table(xtab, P, tid, ENT);
    __syncthreads();
    EPI_INIT();
    for (;;) {
        if (tid == 0) misc[0] = (int)atomicAdd(work_counter, 1u);
        __syncthreads();
        const int win = misc[0];
        __syncthreads();
        if (win >= n_work) break;
        if (win_state[win] == 1) {
            const long long o0 = offs[win];
            const int n = win_lens ? win_lens[win] : (int)(offs[win + 1] - o0);
            const int D = (span - 1 < n - 1) ? span - 1 : n - 1;
            for (int x = tid; x <= n + 1; x += ENT) {
                unsigned char ch = 0;
                if (x >= 1 && x <= n) {
                    ch = seqs[o0 + x - 1];
                    if (ch >= 'a' && ch <= 'z') ch -= 32;
                    if (ch == 'T') ch = 'U';
                }
                seq[x] = ch;
                S[x] = ch == 'A' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : ch == 'U' ? 4 : 0;
            }
            if (tid < ARCH_RB) off[tid] = arch_rowblk_off(tid, n, span);
            __syncthreads();
            if (tid == 0) { S[0] = S[n]; S[n + 1] = S[1]; }
            for (int x = tid + 1; x <= n; x += ENT) pq2[x] = (unsigned char)((S[x] * 6 + (x < n ? (int)S[x + 1] : 5)) * 2);
            special_hairpins(P, seq, n, spec, nc, tid, ENT);
            __syncthreads();
            WinCtx X;
            X.P = P; X.S = S; X.seq = seq; X.f3 = f3; X.spec = spec; X.ldspec = nc; X.n = n; X.D = D; X.E = EP; X.xtab = xtab; X.pq2 = pq2; X.pp = ppart;
            LTab TB;
            TB.carch = slabs + (size_t)win * 3 * slab_shorts; TB.fml = TB.carch + slab_shorts; TB.off = off;
            TB.tb = reinterpret_cast<const unsigned short*>(TB.carch + 2 * slab_shorts);
            fold_epilogue<LTab, ENT>(X, TB, span, f3, starts, lens, btbuf, nc, btstk, misc + 8, win, max_lines, ss_stride, out_lines, out_ss, out_nlines,
                                    out_mfe, out_status);
        }
        __syncthreads();
    }
    EPI_FLUSH();
}

// Epilogue of the vienna-1.8.5 model on the slabs of fold_lds_kernel<1>: exterior sweep, enumeration, full backtracks (interior loops follow the
// trace-back codes), output.  Shares its device code with the generic vienna-1.8.5 kernel (fold185_device.h).
struct LTab185 {
    static constexpr bool kTiled = true;     // 8 x 8-tiled archive with trace-back codes: the patch backtrack applies
    const short* carch;
    const short* fml;
    const unsigned short* tb;
    const int* off;         // LDS: rowblk_off of the tiled archive layout
    int n, D, Dm;
    __device__ __forceinline__ int at(int d, int i) const { return off[(i - 1) >> 3] + ((i - 1) & 7) + 8 * (d - 4); }
    __device__ __forceinline__ int C(int i, int j) const {
        const int d = j - i;
        if (d <= TURN || d > D || i < 1 || j > n) return V_INF;
        const int v = carch[at(d, i)];
        return v == I16_INF ? V_INF : v;
    }
    __device__ __forceinline__ int Mm(int i, int j) const {
        const int d = j - i;
        if (d <= TURN || d > Dm || i < 1 || j > n) return V_INF;
        const int v = (unsigned short)fml[at(d, i)];
        return v == 65535 ? V_INF : v - FML_BIAS;
    }
    __device__ __forceinline__ int TB(int i, int j) const { return tb[at(j - i, i)]; }
};

#ifndef MIRP_EPI185_WGS
#define MIRP_EPI185_WGS 8
#endif
__global__ void __launch_bounds__(ENT, MIRP_EPI185_WGS) fold185_lds_epilogue_kernel(
    const FoldParams* __restrict__ P, const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ win_lens,
    int n_work, int span, const short* __restrict__ slabs, size_t slab_shorts, const int* __restrict__ win_state, unsigned int* __restrict__ work_counter,
    int max_lines, int ss_stride, MirpFoldLine* __restrict__ out_lines, char* __restrict__ out_ss, int* __restrict__ out_nlines,
    int* __restrict__ out_mfe, int* __restrict__ out_status) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nc = LCAP + 8;
    int* f3 = (int*)smem;                                            // nc + 8
    int* starts = f3 + nc + 8;                                       // max_lines
    int* lens = starts + max_lines;                                  // max_lines
    int* btstk = lens + max_lines;                                   // (ENT/64) * 3 * V_BT_STACK
    int* red = btstk + (ENT / 64) * 3 * V_BT_STACK;                  // ENT/64 + 8
    int* misc = red + ENT / 64 + 8;                                  // 4
    int* off = misc + 4;                                             // LDMAX + 2
    short* tetra = (short*)(off + LDMAX + 2);                        // nc
    unsigned char* S = (unsigned char*)(tetra + nc);                 // nc
    unsigned char* seq = S + nc;                                     // nc
    char* btbuf = (char*)(seq + nc);                                 // (ENT/64) * (nc + 8)
    short* dg = (short*)(smem + ((((size_t)(btbuf - (char*)smem) + (ENT / 64) * (nc + 8)) + 15) & ~(size_t)15));   // 80: dangle5 | dangle3
    const int tid = threadIdx.x;
    if (tid < 40) { dg[tid] = (short)P->dangle5[tid / 5][tid % 5]; dg[40 + tid] = (short)P->dangle3[tid / 5][tid % 5]; }
    __syncthreads();
    EPI_INIT();
    for (;;) {
        if (tid == 0) misc[0] = (int)atomicAdd(work_counter, 1u);
        __syncthreads();
        const int win = misc[0];
        __syncthreads();
        if (win >= n_work) break;
        if (win_state[win] == 1) {
            const long long o0 = offs[win];
            const int n = win_lens ? win_lens[win] : (int)(offs[win + 1] - o0);
            for (int x = tid; x <= n + 1; x += ENT) {
                unsigned char ch = 0;
                if (x >= 1 && x <= n) {
                    ch = seqs[o0 + x - 1];
                    if (ch >= 'a' && ch <= 'z') ch -= 32;
                    if (ch == 'T') ch = 'U';
                }
                seq[x] = ch;
                S[x] = ch == 'A' ? 1 : ch == 'C' ? 2 : ch == 'G' ? 3 : ch == 'U' ? 4 : 0;
            }
            for (int x = tid; x < nc + 8; x += ENT) f3[x] = 0;
            if (tid < ARCH_RB) off[tid] = arch_rowblk_off(tid, n, span);
            __syncthreads();
            if (tid == 0) { S[0] = S[n]; S[n + 1] = S[1]; }
            for (int x = tid; x <= n; x += ENT) {
                short b = 0;
                if (x >= 1 && x + 5 <= n)
                    for (int k = 0; k < P->n_tetra; k++) {
                        bool m = true;
                        for (int t = 0; t < 6; t++) m = m && (seq[x + t] == (unsigned char)P->tetra[k][t]);
                        if (m) { b = (short)P->tetraE[k]; break; }
                    }
                tetra[x] = b;
            }
            __syncthreads();
            v185::Ctx<FoldParams> X;
            X.P = P; X.S = S; X.tetra = tetra; X.f3 = f3; X.n = n; X.M = span; X.dg = dg;
            LTab185 T;
            T.carch = slabs + (size_t)win * 3 * slab_shorts; T.fml = T.carch + slab_shorts;
            T.tb = reinterpret_cast<const unsigned short*>(T.carch + 2 * slab_shorts);
            T.off = off; T.n = n; T.D = (span - 1 < n - 1) ? span - 1 : n - 1; T.Dm = (span < n - 1) ? span : n - 1;
            v185::epilogue<FoldParams, LTab185, ENT>(X, T, f3, starts, lens, btstk, red, btbuf, nc, win, max_lines, ss_stride, out_lines, out_ss, out_nlines,
                                                     out_mfe, out_status);
        }
        __syncthreads();
    }
    EPI_FLUSH();
}

size_t fold185_lds_epilogue_bytes(int max_lines) {
    const size_t nc = LCAP + 8;
    size_t b = sizeof(int) * (nc + 8 + 2 * (size_t)max_lines + (ENT / 64) * 3 * V_BT_STACK + ENT / 64 + 8 + 4 + LDMAX + 2);
    b += sizeof(short) * nc + 2 * nc + (ENT / 64) * (nc + 8);
    return ((b + 15) & ~(size_t)15) + 16 + 80 * sizeof(short);
}

size_t fold_lds_epilogue_bytes(int max_lines) {
    const int nc = LCAP + 8;
    size_t b = sizeof(int) * (nc + 2 * (size_t)max_lines + (ENT / 64) * 3 * BT_STACK + 16 + LDMAX + 2) + sizeof(short) * 3 * nc + 2 * (size_t)nc + (ENT / 64) * (size_t)nc;
    b = (b + 15) & ~(size_t)15;
    return b + sizeof(EpiTables) + 16 + sizeof(short) * XTAB_N + nc + sizeof(short) * nc;
}

size_t fold_lds_bytes(int max_lines) { (void)max_lines; return lds_layout<0>().total; }      // the largest workgroup of the path (dense pass)
int fold_lds_max_n() { return LCAP - 2; }
int fold_lds_gen_wing_d() { return 5; }      // GEN_WD of fold_lds_kernel<0>
int fold_lds_max_span() { return LSPAN; }

// ---- launches (mirp_fold.cpp composes them).  One fill pass: a kernel of fold_lds_kernel's signature, its workgroup, its LDS and how many of its
// workgroups a CU holds -- the grid is that many per CU the caller asks for, at most one per window.
using FillKernel = decltype(&fold_lds_kernel<0, false, LNT>);
struct FillPass { FillKernel kernel; int threads; size_t lds; int per_cu; };
// The dense pass: the dense split loop, over the windows a pool pass handed over (pool overflow, no room for a pool: none on the benchmark inputs, the
// launch then finds an empty list) or over every window (mirp_set_fold_split_path(1): tests, A/B timing).
static FillPass dense_pass(int model) {
    return model ? FillPass{fold_lds_kernel<1, false>, LNT, lds_layout<1>().total, 1} : FillPass{fold_lds_kernel<0, false>, LNT, lds_layout<0>().total, 1};
}
// The candidate-pool pass: sparse multiloop splits, the product's first pass.  Default model: two 512-thread workgroups per CU.  vienna-1.8.5: with
// dangles 1 every pair gives up to four strictly pair-realised fML cells ((i,j), (i-1,j), (i,j+1), (i-1,j+1)), i.e. about four times the candidate
// cells of the default model (3,142 per benchmark window: a cell pool overflowed for most windows, 161 ms = both passes); the pool of that
// instantiation holds PAIRS instead (1,283 per window, 8-byte entries: splits_sparse185).
static FillPass pool_pass(int model) {
    return model ? FillPass{fold_lds_kernel<1, true>, LNT, lds_layout<1, true>().total, 1} : FillPass{fold_lds_kernel<0, true, LNT2>, LNT2, lds_layout<0, true, true>().total, 2};
}

// counter: the work counter of the block the pass draws from; from_list: over the block's dense list, which it may itself extend, instead of every window
static hipError_t launch_fill(const FillPass& f, hipStream_t stream, int grid, const FoldLdsArgs& a, int counter, bool from_list) {
    unsigned int* const list_len = a.ctl + FOLD_CTL_DENSE_LEN;
    hipLaunchKernelGGL(f.kernel, dim3(std::min(a.n_work, f.per_cu * grid)), dim3(f.threads), f.lds, stream, a.P, a.seqs, a.offs, a.lens, a.n_work, a.win_base, a.span, a.slabs,
                       a.slab_shorts, a.win_state, a.ctl + counter, a.fallback_list, a.fallback_count, a.max_lines, a.ss_stride, a.out_lines, a.out_ss, a.out_nlines, a.out_mfe,
                       a.out_status, a.light_clocks, a.dbg_cycles, from_list ? (const int*)a.dense_list : nullptr, from_list ? (const unsigned int*)list_len : nullptr,
                       a.dense_list, list_len);
    return hipGetLastError();
}

hipError_t launch_fold_lds_pool(hipStream_t stream, int model, int grid, const FoldLdsArgs& a) { return launch_fill(pool_pass(model), stream, grid, a, FOLD_CTL_FILL, false); }

hipError_t launch_fold_lds_dense(hipStream_t stream, int model, int grid, const FoldLdsArgs& a, bool every_window) {
    return launch_fill(dense_pass(model), stream, grid, a, every_window ? FOLD_CTL_FILL : FOLD_CTL_DENSE, !every_window);
}

template <class K>
static hipError_t launch_epilogue(K kernel, size_t lds, hipStream_t stream, int grid, const FoldLdsArgs& a) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(ENT), lds, stream, a.P, a.seqs, a.offs, a.lens, a.n_work, a.span, a.slabs, a.slab_shorts, a.win_state, a.ctl + FOLD_CTL_EPILOGUE,
                       a.max_lines, a.ss_stride, a.out_lines, a.out_ss, a.out_nlines, a.out_mfe, a.out_status);
    return hipGetLastError();
}

hipError_t launch_fold_lds_epilogue(hipStream_t stream, int model, int grid, const FoldLdsArgs& a) {
    return model ? launch_epilogue(fold185_lds_epilogue_kernel, fold185_lds_epilogue_bytes(a.max_lines), stream, grid, a)
                 : launch_epilogue(fold_lds_epilogue_kernel, fold_lds_epilogue_bytes(a.max_lines), stream, grid, a);
}

// What the launches above rely on, on the current device: the LDS every fill pass and, where max_lines asks for more than 64 KB, the vienna-1.8.5
// epilogue may take, and two workgroups of the default model's candidate-pool pass per CU -- the whole point of its LDS layout: refuse to run at half
// the occupancy if a later change of its LDS or register budget no longer lets two of them share a CU.
hipError_t fold_lds_prepare(int max_lines) {
    for (const FillPass& f : {pool_pass(0), pool_pass(1), dense_pass(0), dense_pass(1)})
        if (hipError_t e = hipFuncSetAttribute((const void*)f.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds)) return e;
    if (const size_t el = fold185_lds_epilogue_bytes(max_lines); el > 64 * 1024)
        if (hipError_t e = hipFuncSetAttribute((const void*)fold185_lds_epilogue_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)el)) return e;
    const FillPass two = pool_pass(0);
    int per_cu = 0;
    if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)two.kernel, two.threads, two.lds)) return e;
    if (per_cu != two.per_cu) {
        std::fprintf(stderr, "[mirp] fold_lds_kernel<0, true, %d>: %d workgroups per CU instead of 2 (%zu bytes of LDS)\n", LNT2, per_cu > 0 ? per_cu : -1, two.lds);
        return hipErrorLaunchOutOfResources;
    }
    return hipSuccess;
}

// A SIMD of gfx950 has 512 VGPRs handed out in blocks of 8 and 8 wave slots; a CU has 160 KB of LDS in granules of 1280 bytes.  A workgroup of the
// candidate-pool pass puts LNT2 / 256 waves on every SIMD, one of the epilogue ENT / 256.
int fold_lds_overlap_epi_wgs(int max_lines) {
    hipFuncAttributes fa, ea;
    if (hipFuncGetAttributes(&fa, (const void*)fold_lds_kernel<0, true, LNT2>) != hipSuccess) return -1;
    if (hipFuncGetAttributes(&ea, (const void*)fold_lds_epilogue_kernel) != hipSuccess) return -1;
    const int fr = (fa.numRegs + 7) & ~7, er = (ea.numRegs + 7) & ~7;
    const int fw = 2 * (LNT2 / 256), ew = ENT / 256 > 0 ? ENT / 256 : 1;
    if (fr <= 0 || er <= 0 || fw * fr > 512 || fw > 8) return 0;
    const int by_regs = (512 - fw * fr) / (er * ew), by_slots = (8 - fw) / ew;
    const unsigned fl = LDS_GRANULES((unsigned)(lds_layout<0, true, true>().total + fa.sharedSizeBytes));
    const unsigned el = LDS_GRANULES((unsigned)(fold_lds_epilogue_bytes(max_lines) + ea.sharedSizeBytes));
    const int by_lds = 2 * fl > 128 ? 0 : (int)((128 - 2 * fl) / el);
    return std::min(std::min(by_regs, MIRP_OVERLAP_EPI_WGS), std::min(by_slots, by_lds));      // (no more than the layout was made for)
}

#ifdef MIRP_DIAG
void fold_lds_epi_clocks_print() {
    unsigned long long h[32];
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_epi_clk), sizeof(h));
    const char* nm[14] = {"f3 sweep", "enumeration", "partner scan", "backtrack", "output", "loop tail", "barrier", "containment",
                          "sweep: issue+init+barrier", "sweep: load wait", "sweep: step 1", "sweep: barrier 2", "sweep: step 2", "sweep: barrier 3"};
    for (int k = 0; k < 14; k++) std::fprintf(stderr, "[mirp epi clocks] %-14s %llu\n", nm[k], h[k]);
    const char* cn[10] = {"ext partner scan rounds", "ml segment pops", "ml pair checks", "ml split rounds (segment)", "helix line fetches", "line-end c fetches",
                          "line-end code fetches", "ml split rounds (closing)", "short-backtrack scan rounds", "structures"};
    for (int k = 0; k < 10; k++) std::fprintf(stderr, "[mirp epi counts] %-28s %llu\n", cn[k], h[16 + k]);
    unsigned long long z[32] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_epi_clk), z, sizeof(z));
}
#endif

size_t fold_lds_slab_shorts(int n_cap) {   // tiled archive of one table for windows up to n_cap at the largest span (whole 128-byte tiles)
    return (size_t)arch_rowblk_off(ARCH_RB, n_cap < LCAP ? n_cap : LCAP, LDMAX + 1) + 64;
}

}  // namespace mirp

// Accessibility of an interval of many short windows (mirp_unpaired_batch, targets -u): Z of §23 and Z_open, the same inside
// program with Qb(i,j) = 0 wherever i or j lies in the interval, carried through one pass as the two halves of every cell.
//
// One wave folds one window of n <= 128 nt; its lanes sit on the cells of an anti-diagonal d = j - i (two cells per lane above 64 nt), the
// diagonals run from d = 4 outwards with a wave barrier between them, then the exterior prefixes Q5 run left to right.  Every value is a plain
// FP64 Boltzmann weight (§24, "Range": at 128 nt the largest ln Q is about 320 of FP64's 709): a loop's factor is exp(EN_G * its integer energy),
// taken once and multiplied into both halves; only the two final values take a log.  A sum is walked by one lane in a fixed order (hairpin,
// interior loops by n1 then n2, multiloop; the splits k ascending); the exterior sum of a column is one partial per lane (k = lane, lane + 64)
// folded by the xor butterfly, in which a + b = b + a makes every lane hold the same bits.  So a window's three doubles depend on nothing but
// the window: no atomics, no dependence on the grid, the bins or the slab's place.
//
// Tables, as {free, open} pairs of doubles stored by diagonals (row d holds the cells (i, i + d), i < n - d, from row 3, which is zero): Qb, Qm
// and Qm1 are read at any distance and live in the wave's slab, 3 (n - 2)(n - 3) / 2 cells of 16 bytes; U is read one diagonal back and Qmm two,
// so they are rings of 2 and 3 rows.  The slab of a launch is sized by the launch's n_max (the host bins the windows by length class) and lies in
// LDS when the block's LDS stays within UP_LDS_BYTES (two blocks per CU; up to 56 nt), in a wave-private stretch of device memory otherwise:
// three FP64 tables of two halves take 91 KB at 64 nt and 378 KB at 128.  The arithmetic is the same in both places.  A block is one wave: there is no block barrier.
//
// Two sources of windows share the kernel: UpBatch (mirp_unpaired_batch: coded windows, offsets, intervals, and the order the host binned them
// in) and UpSites (targets -u: the sorted keys of a pass; the window is the site's interval on the forward target extended by the flanks and
// clipped to the contig, reverse-complemented on the minus strand; keys that -k cuts are not folded).  UpSites reads the keys as DxSites does
// (duplex_kernels.hip), through site_kept, SiteKey and site_contig of site_keys.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mirp_ctx.h"
#include "fold_device.h"
#include "ensemble_device.h"
#include "site_keys.h"

namespace mirp {

constexpr int UP_MAX = MIRP_UNPAIRED_MAX;
constexpr int UP_LDS_BYTES = 80 * 1024;      // a block whose tables fit this keeps its slab in LDS: two blocks on a CU's 160 KiB

struct alignas(16) UpCell { double f, o; };

struct UpAux {
    EnTables T;
    alignas(16) UpCell q5[UP_MAX];
    unsigned char S[UP_MAX];
};
static_assert(sizeof(UpAux) % 16 == 0, "the rings and the slab behind it stay 16-byte aligned");

// cells of one table of a window of n nt (rows 3 .. n - 1), and the first cell of row d >= 3
__host__ __device__ constexpr int up_cells(int n) { return n > 3 ? (n - 2) * (n - 3) / 2 : 0; }
__device__ __forceinline__ int up_off(int n, int d) { return (d - 3) * n - ((d * (d - 1)) >> 1) + 3; }

__device__ __forceinline__ void up_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // the block is this wave; the scope makes the slab's stores in device memory wait as well
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ double up_wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double up_bf(int e) { return exp(EN_G * (double)e); }

// ---------------------------------------------------------------- the window of job q: where its result goes, length, interval (0-based), this lane's two codes
struct UpBatch {
    const unsigned char* codes; const long long* offs; const int* lo; const int* hi; const int* order;
    __device__ bool load(long long q, int lane, long long* rec, int* n, int* lo0, int* hi0, int* c0, int* c1) const {
        const int w = order[q];
        const long long at = offs[w];
        *rec = w;
        *n = (int)(offs[w + 1] - at);
        *lo0 = lo[w] - 1;
        *hi0 = hi[w] - 1;
        *c0 = lane < *n ? (int)codes[at + lane] : 0;
        *c1 = lane + 64 < *n ? (int)codes[at + lane + 64] : 0;
        return true;
    }
};

template <bool BULGE>
struct UpSites {
    DxTargets T;
    const unsigned long long* keys;
    long long n, k;                         // keys of the pass; -k (0 = all)
    const unsigned long long* emitted;
    int up, down;
    __device__ bool load(long long q, int lane, long long* rec, int* n_out, int* lo0, int* hi0, int* c0, int* c1) const {
        *rec = q;
        if (!site_kept(keys, q, k, emitted, SiteKey<BULGE>::shift)) return false;
        const SiteKey<BULGE> K(keys[q]);
        const int strand = K.strand;
        const unsigned long long g = K.g;
        const int len = K.len(T.mi[K.mloc].L);
        const int c = site_contig(T.cstart, T.n_contigs, g);
        // forward bases before / behind the interval: up / down on the plus strand, the other way round on the minus strand
        const unsigned long long before = strand ? (unsigned long long)down : (unsigned long long)up, behind = strand ? (unsigned long long)up : (unsigned long long)down;
        const unsigned long long room0 = g - T.cstart[c], room1 = T.cstart[c + 1] - (g + len);
        const unsigned long long w0 = g - (before < room0 ? before : room0), w1 = g + len + (behind < room1 ? behind : room1);      // [w0, w1)
        const int nw = (int)(w1 - w0);
        *n_out = nw;
        *lo0 = strand ? (int)(w1 - (g + len)) : (int)(g - w0);
        *hi0 = *lo0 + len - 1;
        int y[2];
        for (int h = 0; h < 2; h++) {
            const int x = lane + 64 * h;
            y[h] = 0;
            if (x < nw) {
                const unsigned long long p = strand ? w1 - 1 - x : w0 + x;
                const unsigned base = tg_base(T.pk, p);
                y[h] = (T.amb[p >> 5] >> (p & 31)) & 1u ? 0 : (int)(strand ? 3u - base : base) + 1;
            }
        }
        *c0 = y[0];
        *c1 = y[1];
        return true;
    }
};

// ---------------------------------------------------------------- the kernel
// The record of a window goes to out[rec], or with out null upe x 1000 rounded to nearest to out_milli[rec] (targets -u).
// LDS: UpAux, the rings (5 rows of `stride` cells), and with LDS_SLAB the slab of 3 * cells cells; otherwise block b's slab is g_slab + b * 3 * cells.
template <class SRC, bool LDS_SLAB>
__global__ __launch_bounds__(64) void unpaired_kernel(SRC src, long long n_jobs, const FoldParams* __restrict__ P, int n_max, int stride, int cells,
                                                      UpCell* __restrict__ g_slab, MirpUnpairedRec* __restrict__ out, int* __restrict__ out_milli) {
    extern __shared__ __align__(16) unsigned char up_smem[];
    UpAux& A = *(UpAux*)up_smem;
    UpCell* ringU = (UpCell*)(up_smem + sizeof(UpAux));      // row d & 1
    UpCell* ringM = ringU + 2 * stride;                       // row d % 3
    UpCell* slab = LDS_SLAB ? ringM + 3 * stride : g_slab + (size_t)blockIdx.x * 3 * (size_t)cells;
    UpCell *Qb = slab, *Qm = slab + cells, *Qm1 = slab + 2 * (size_t)cells;
    const int lane = threadIdx.x;
    en_stage(&A.T, A.S, P, nullptr, 0, lane, 64);
    const EnTables& T = A.T;
    unsigned char* S = A.S;
    for (long long q = blockIdx.x; q < n_jobs; q += gridDim.x) {
        long long rec;
        int n, lo, hi, c0, c1;
        const bool run = src.load(q, lane, &rec, &n, &lo, &hi, &c0, &c1);
        n = __builtin_amdgcn_readfirstlane(n);
        lo = __builtin_amdgcn_readfirstlane(lo);
        hi = __builtin_amdgcn_readfirstlane(hi);
        if (!run || n < 1 || n > n_max || lo < 0 || hi < lo || hi >= n) {      // a key that -k cuts; otherwise never with the host's checks: no cell outside the slab
            if (lane == 0) {
                if (out) out[rec] = MirpUnpairedRec{0.0, 0.0, 0.0};
                else out_milli[rec] = 0;
            }
            continue;
        }
        up_sync();                          // the previous window of this wave is done with the tables
        S[lane] = (unsigned char)c0;
        S[lane + 64] = (unsigned char)c1;
        for (int x = lane; x < 5 * stride; x += 64) ringU[x] = UpCell{0.0, 0.0};
        for (int x = lane; x < n - 3; x += 64) Qm1[x] = UpCell{0.0, 0.0};
        up_sync();
        // ---- inside
        for (int d = 4; d < n; d++) {
            const int row = up_off(n, d), row1 = up_off(n, d - 1);
            UpCell* Ud = ringU + (d & 1) * stride;
            const UpCell* U1 = ringU + ((d - 1) & 1) * stride;
            UpCell* Md = ringM + (d % 3) * stride;
            const UpCell* M2 = ringM + ((d - 2) % 3) * stride;
            for (int i = lane; i < n - d; i += 64) {
                const int j = i + d;
                const int type = pair_type(S[i], S[j]);
                UpCell q1 = Qm1[row1 + i];
                if (type) {
                    const double h = up_bf(en_hairpin(T, P, S, i, j, type));
                    double f = h, o = h;
                    const int n1max = d - 6 < MIRP_MAXLOOP ? d - 6 : MIRP_MAXLOOP;          // q - p >= 4 with n2 = 0
                    for (int n1 = 0; n1 <= n1max; n1++) {
                        const int p = i + 1 + n1;
                        int n2max = MIRP_MAXLOOP - n1;
                        if (n2max > d - 6 - n1) n2max = d - 6 - n1;
                        for (int n2 = 0; n2 <= n2max; n2++) {
                            const int qq = j - 1 - n2;
                            const int t2 = pair_type(S[p], S[qq]);
                            if (!t2) continue;
                            const UpCell in = Qb[up_off(n, d - 2 - n1 - n2) + p];
                            if (in.f == 0.0) continue;
                            const double w = up_bf(en_intloop(T, P, n1, n2, type, rtype_of(t2), S[i + 1], S[j - 1], S[p - 1], S[qq + 1]));
                            f += w * in.f;
                            o += w * in.o;
                        }
                    }
                    const double m = up_bf(T.ML_closing + en_mlstem(T, rtype_of(type), S[j - 1], S[i + 1]));
                    const UpCell mm = M2[i + 1];
                    f += m * mm.f;
                    o += m * mm.o;
                    if ((i >= lo && i <= hi) || (j >= lo && j <= hi)) o = 0.0;
                    Qb[row + i] = UpCell{f, o};
                    const double s = up_bf(en_mlstem(T, type, i > 0 ? S[i - 1] : -1, j < n - 1 ? S[j + 1] : -1));
                    q1.f += f * s;
                    q1.o += o * s;
                } else Qb[row + i] = UpCell{0.0, 0.0};
                const UpCell u1 = U1[i + 1];
                const UpCell u = UpCell{u1.f + q1.f, u1.o + q1.o};
                double mf = 0.0, mo = 0.0;
                for (int k = i + 5; k <= j - 4; k++) {
                    const UpCell a = Qm[up_off(n, k - 1 - i) + i], b = Qm1[up_off(n, j - k) + k];
                    mf += a.f * b.f;
                    mo += a.o * b.o;
                }
                Qm1[row + i] = q1;
                Ud[i] = u;
                Md[i] = UpCell{mf, mo};
                Qm[row + i] = UpCell{u.f + mf, u.o + mo};
            }
            up_sync();
        }
        // ---- exterior prefixes: q5[j] = the partition functions of [0, j]
        for (int j = 0; j < n; j++) {
            double f = 0.0, o = 0.0;
            for (int k = lane; k <= j - 4; k += 64) {
                const int t = pair_type(S[k], S[j]);
                if (t) {
                    const double w = up_bf(en_extloop(T, t, k > 0 ? S[k - 1] : -1, j < n - 1 ? S[j + 1] : -1));
                    const UpCell b = Qb[up_off(n, j - k) + k];
                    const UpCell pre = k > 0 ? A.q5[k - 1] : UpCell{1.0, 1.0};
                    f += pre.f * b.f * w;
                    o += pre.o * b.o * w;
                }
            }
            f = up_wave_sum(f);
            o = up_wave_sum(o);
            if (lane == 0) {
                const UpCell pre = j > 0 ? A.q5[j - 1] : UpCell{1.0, 1.0};
                A.q5[j] = UpCell{pre.f + f, pre.o + o};
            }
            up_sync();
        }
        if (lane == 0) {
            const UpCell z = A.q5[n - 1];
            MirpUnpairedRec r;
            r.efe = 0.0 - EN_KT * log(z.f);
            r.efe_open = 0.0 - EN_KT * log(z.o);
            r.upe = r.efe_open - r.efe;
            if (out) out[rec] = r;
            else out_milli[rec] = (int)floor(r.upe * 1000.0 + 0.5);
        }
    }
}

}  // namespace mirp

namespace {

constexpr size_t up_lds_fixed(int stride) { return sizeof(mirp::UpAux) + sizeof(mirp::UpCell) * 5 * (size_t)stride; }
constexpr size_t up_lds_all(int n) { return up_lds_fixed((n + 7) / 8 * 8) + sizeof(mirp::UpCell) * 3 * (size_t)mirp::up_cells(n); }
constexpr int up_lds_longest() {          // the longest window whose slab stays in LDS
    int n = 1;
    while (n < mirp::UP_MAX && up_lds_all(n + 1) <= (size_t)mirp::UP_LDS_BYTES) n++;
    return n;
}

template <class SRC>
int up_launch(mirp_ctx* c, const SRC& src, long long n, int n_max, MirpUnpairedRec* d_out, int* d_milli) {
    using namespace mirp;
    if (n <= 0) return 0;
    if (n_max < 1 || n_max > UP_MAX) return fail(c, -5, "unpaired: a window longer than 128 nt reached the kernel");
    const int stride = (n_max + 7) / 8 * 8, cells = up_cells(n_max);
    const size_t fixed = up_lds_fixed(stride), slab = sizeof(UpCell) * 3 * (size_t)cells;
    static_assert(sizeof(UpAux) + sizeof(UpCell) * 5 * UP_MAX <= 32 * 1024 && UP_LDS_BYTES <= 160 * 1024, "LDS budget");
    if (fixed + slab <= (size_t)mirp::UP_LDS_BYTES) {
        static size_t lds_set = 0;          // per instantiation
        if (fixed + slab > lds_set) {
            HIPCHK(c, hipFuncSetAttribute((const void*)unpaired_kernel<SRC, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(fixed + slab)));
            lds_set = fixed + slab;
        }
        const long long resident = (long long)c->n_cu * std::min<long long>(32, (160 * 1024) / (long long)(fixed + slab));
        c->note_jobs_per_slot(1, n, std::min(n, 2 * resident));
        hipLaunchKernelGGL((unpaired_kernel<SRC, true>), dim3((unsigned)std::min(n, 2 * resident)), dim3(64), fixed + slab, c->stream, src, n,
                           (const FoldParams*)c->d_params, n_max, stride, cells, (UpCell*)nullptr, d_out, d_milli);
    } else {
        const long long blocks = std::min<long long>(n, (long long)c->n_cu * 4);          // as many wave-private slabs
        if (c->up_slab.ensure(slab * (size_t)blocks)) return fail(c, -6, "unpaired: device allocation failed (the slabs)");
        c->note_jobs_per_slot(1, n, blocks);
        hipLaunchKernelGGL((unpaired_kernel<SRC, false>), dim3((unsigned)blocks), dim3(64), fixed, c->stream, src, n, (const FoldParams*)c->d_params, n_max,
                           stride, cells, (UpCell*)c->up_slab.p, d_out, d_milli);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

}  // namespace

// the launches of the batch are sized by classes of length, so that where a window's tables lie depends on its length alone: the multiples of 8
// and the longest length of the LDS slab
int mirp_unpaired_class(int n) {
    const int up8 = (n + 7) / 8 * 8;
    return n <= up_lds_longest() && up8 > up_lds_longest() ? up_lds_longest() : up8;
}

// the longest window whose slab lies in LDS (for tests of the lengths around the hand-over to device memory)
extern "C" int mirp_unpaired_lds_longest(void) { return up_lds_longest(); }

int mirp_device_unpaired_batch(mirp_ctx* c, const unsigned char* d_codes, const long long* d_offs, const int* d_lo, const int* d_hi, const int* d_order,
                               long long n, int n_max, MirpUnpairedRec* d_recs) {
    return up_launch(c, mirp::UpBatch{d_codes, d_offs, d_lo, d_hi, d_order}, n, n_max, d_recs, nullptr);
}

int mirp_device_unpaired_sites(mirp_ctx* c, const DxTargets& T, bool bulge, const unsigned long long* d_keys, long long n, long long max_sites,
                               const unsigned long long* d_emitted, int longest, int up, int down, int* d_milli) {
    // the interval (at most 33 bases: 32 and an unpaired one) and the flanks (up + down <= 95): <= 128
    if (up < 0 || down < 0 || up + down > 95 || longest < 1 || longest > 33) return fail(c, -5, "unpaired: flanks or an interval outside the limits reached the kernel");
    if (bulge) return up_launch(c, mirp::UpSites<true>{T, d_keys, n, max_sites, d_emitted, up, down}, n, longest + up + down, nullptr, d_milli);
    return up_launch(c, mirp::UpSites<false>{T, d_keys, n, max_sites, d_emitted, up, down}, n, longest + up + down, nullptr, d_milli);
}

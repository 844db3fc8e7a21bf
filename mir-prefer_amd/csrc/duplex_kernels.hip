// Two-strand (intermolecular) minimum free energy fold: the model of DESIGN.md §21 -- the RNAduplex recursion on the Turner-2004 tables with
// dangles = 2, energies in 0.01 kcal/mol.  The tables are the context's resident FoldParams of the vienna-2.1.2 model and the loop energies are
// e_intloop / e_extloop of fold_device.h; mirp_set_fold_model does not change the result (there is no Turner-1999 duplex model).
//
// One wave folds one duplex of strands a (la <= 64) and b (lb <= 64), both 5'->3'; lane j owns column j.
//   fill    rows i = 0 .. la - 1 in order: c[i][j] = min(410 + E_ext, min over k < i, l > j, (i - k - 1) + (l - j - 1) <= 30 of c[k][l] + E_int).
//           Every cell of a row depends on earlier rows only, so a row is one step of the wave.  c lives in a wave-private LDS slab of
//           max_la x max_lb ints (the largest shapes of the launch); next to it the two strands (codes 0..4 = N A C G U, -1 beyond either end) and
//           one 64-bit mask per row of the cells that hold a pair, so that a lane walks the set bits of (mask[k] >> (j + 1)) and reads no cell
//           at INF.  Cells whose pair type is 0 are skipped.
//   end     f(i, j) = c[i][j] + E_ext of the inner end, tracked per lane while the rows are filled (the first minimum: the smallest i), then
//           reduced over the wave: the minimal f, the smallest i, the largest j.
//   trace   from the end cell, k = i - 1 downwards with the lanes on l: the first row with a matching predecessor, its smallest l.  The chain is
//           nested, so the two 64-bit masks of the paired positions determine it; they and min(0, f) are the result.
// Waves never wait on each other: a block is DX_WAVES independent waves, each with its own slab, and there is no block barrier.
//
// Three sources of strands share the kernel: DxPairs (mirp_duplex_batch: coded strands and offsets), DxPerfect (a miRNA against its reverse
// complement, N stays N: `mfe_perfect` of targets -e) and DxSites (targets -e: the sorted keys of a pass; a = the miRNA, b = the site's interval on
// the forward target plus one base on each side where the contig has one, an ambiguous one as N, reverse-complemented on the minus strand; keys
// that -k cuts are not folded).  DxSites reads the keys through site_keys.h: site_kept is the cut that site_size_kernel applies (site_lines.h),
// SiteKey the decoder of both key layouts, site_contig the contig lookup.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "mirp_ctx.h"
#include "fold_device.h"
#include "site_keys.h"

namespace mirp {

#define DX_WAVES 4
#define DX_INIT 410                  // intermolecular initiation (DuplexInit)
#define DX_AUX_INTS (2 * 66 + 2 * 64)    // per wave behind the slab: sa[66], sb[66] (index p + 1), the row masks as two ints each

__device__ __forceinline__ void dx_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int dx_wave_min(int v) {
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int dx_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------- the strands of job q: lengths (wave-uniform) and this lane's codes (-1 past the end)
struct DxPairs {
    const unsigned char* a; const long long* aoff; const unsigned char* b; const long long* boff;
    __device__ bool load(long long q, int lane, int* la, int* lb, int* ca, int* cb) const {
        const long long a0 = aoff[q], b0 = boff[q];
        *la = (int)(aoff[q + 1] - a0);
        *lb = (int)(boff[q + 1] - b0);
        *ca = lane < *la ? (int)a[a0 + lane] : -1;
        *cb = lane < *lb ? (int)b[b0 + lane] : -1;
        return true;
    }
};

struct DxPerfect {
    const unsigned char* mcodes;            // 32 per miRNA: 0..3 = A C G U, 4 = unknown
    const TgMirna* mi;
    __device__ bool load(long long q, int lane, int* la, int* lb, int* ca, int* cb) const {
        const int L = mi[q].L;
        *la = *lb = L;
        const unsigned x = lane < L ? mcodes[32 * q + lane] : 4u, y = lane < L ? mcodes[32 * q + (L - 1 - lane)] : 4u;
        *ca = lane < L ? (x < 4 ? (int)x + 1 : 0) : -1;
        *cb = lane < L ? (y < 4 ? 4 - (int)y : 0) : -1;
        return true;
    }
};

template <bool BULGE>
struct DxSites {
    DxTargets T;
    const unsigned long long* keys;
    long long n, k;                         // keys of the pass; -k (0 = all)
    const unsigned long long* emitted;
    __device__ bool load(long long q, int lane, int* la, int* lb, int* ca, int* cb) const {
        if (!site_kept(keys, q, k, emitted, SiteKey<BULGE>::shift)) return false;
        const SiteKey<BULGE> K(keys[q]);
        const int mloc = K.mloc, strand = K.strand;
        const unsigned long long g = K.g;
        const int L = T.mi[mloc].L, len = K.len(L);
        const int c0 = site_contig(T.cstart, T.n_contigs, g);
        const unsigned long long lo = g > T.cstart[c0] ? g - 1 : g, hi = g + len < T.cstart[c0 + 1] ? g + len : g + len - 1;
        const int nb = (int)(hi - lo) + 1;
        *la = L;
        *lb = nb;
        const unsigned x = lane < L ? T.mcodes[32 * ((long long)T.mbase + mloc) + lane] : 4u;
        *ca = lane < L ? (x < 4 ? (int)x + 1 : 0) : -1;
        int y = -1;
        if (lane < nb) {
            const unsigned long long p = strand ? hi - lane : lo + lane;
            const unsigned base = tg_base(T.pk, p);
            y = (T.amb[p >> 5] >> (p & 31)) & 1u ? 0 : (int)(strand ? 3u - base : base) + 1;
        }
        *cb = y;
        return true;
    }
};

// ---------------------------------------------------------------- the kernel
template <class SRC>
__global__ __launch_bounds__(64 * DX_WAVES) void duplex_kernel(SRC src, long long n, const FoldParams* __restrict__ P, int rows, int stride,
                                                               int* __restrict__ out_mfe, unsigned long long* __restrict__ out_ma,
                                                               unsigned long long* __restrict__ out_mb, unsigned long long* __restrict__ evals) {
    extern __shared__ __align__(16) int dx_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* c = dx_smem + (size_t)wave * ((size_t)rows * stride + DX_AUX_INTS);
    int* sa = c + (size_t)rows * stride;    // sa[p + 1] = a[p], -1 at p = -1 and p >= la
    int* sb = sa + 66;
    int* rmask = sb + 66;                   // row k: bits 0..31 at [2 k], 32..63 at [2 k + 1]
    unsigned long long n_eval = 0;
    for (long long q = (long long)blockIdx.x * DX_WAVES + wave; q < n; q += (long long)gridDim.x * DX_WAVES) {
        int la, lb, ca, cb;
        const bool run = src.load(q, lane, &la, &lb, &ca, &cb);
        if (!run) {                         // wave-uniform: a key that -k cuts
            if (lane == 0) { out_mfe[q] = 0; if (out_ma) { out_ma[q] = 0; out_mb[q] = 0; } }
            continue;
        }
        la = dx_uniform(la);
        lb = dx_uniform(lb);
        if (la > rows || lb > stride || la < 1 || lb < 1) {      // never with the host's checks: no cell outside the slab
            if (lane == 0) { out_mfe[q] = 0; if (out_ma) { out_ma[q] = 0; out_mb[q] = 0; } }
            continue;
        }
        dx_sync();                          // the previous duplex of this wave is done with the slab
        sa[lane + 1] = ca;
        sb[lane + 1] = cb;
        if (lane == 0) { sa[0] = -1; sb[0] = -1; sa[65] = -1; sb[65] = -1; }
        dx_sync();
        const int bj = cb, bjm = sb[lane], bjp = sb[lane + 2];   // b[j], b[j - 1], b[j + 1]
        int f_best = MIRP_INF, i_best = 0;
        // ---- fill
        for (int i = 0; i < la; i++) {
            const int ai = sa[i + 1], si = sa[i];
            const int t = lane < lb ? pair_type(ai, bj) : 0;
            int best = MIRP_INF;
            if (t) {
                const int t2 = rtype_of(t);
                best = DX_INIT + e_extloop(P, t, si, bjp);
                const int k0 = i - 1 - MIRP_MAXLOOP > 0 ? i - 1 - MIRP_MAXLOOP : 0;
                for (int k = i - 1; k >= k0; k--) {
                    const int n1 = i - k - 1;
                    const int room = min(MIRP_MAXLOOP - n1, lb - 2 - lane);          // n2 = l - j - 1 runs 0 .. room
                    if (room < 0) continue;
                    unsigned long long m = ((unsigned long long)(unsigned)rmask[2 * k] | ((unsigned long long)(unsigned)rmask[2 * k + 1] << 32)) >> (lane + 1);
                    if (room < 63) m &= (1ull << (room + 1)) - 1ull;
                    const int ak = sa[k + 1], sk1 = sa[k + 2];
                    const int* ck = c + (size_t)k * stride + lane + 1;
                    while (m) {
                        const int n2 = __ffsll((unsigned long long)m) - 1;
                        m &= m - 1;
                        const int l = lane + 1 + n2;
                        const int e = ck[n2] + e_intloop(P, n1, n2, pair_type(ak, sb[l + 1]), t2, sk1, sb[l], si, bjp);
                        best = e < best ? e : best;
                        n_eval++;
                    }
                }
                const int f = best + e_extloop(P, t2, bjm, sa[i + 2]);
                if (f < f_best) { f_best = f; i_best = i; }
            }
            if (lane < lb) c[(size_t)i * stride + lane] = best;
            const unsigned long long paired = __ballot(t != 0);
            if (lane == 0) { rmask[2 * i] = (int)(unsigned)paired; rmask[2 * i + 1] = (int)(unsigned)(paired >> 32); }
            dx_sync();
        }
        // ---- end cell: the minimal f, the smallest i, the largest j
        const int f_min = dx_wave_min(f_best);
        unsigned long long ma = 0, mb = 0;
        if (f_min < 0) {
            int i = dx_uniform(dx_wave_min(f_best == f_min ? i_best : 64));
            int j = 63 - __builtin_clzll(__ballot(f_best == f_min && i_best == i));
            // ---- trace back
            for (;;) {
                ma |= 1ull << i;
                mb |= 1ull << j;
                const int cij = c[(size_t)i * stride + j];
                const int t2 = rtype_of(pair_type(sa[i + 1], sb[j + 1]));
                const int si = sa[i], sq = sb[j + 2];
                int nk = -1, nl = -1;
                for (int k = i - 1; k >= 0 && i - k - 1 <= MIRP_MAXLOOP; k--) {
                    const int n1 = i - k - 1, n2 = lane - j - 1;
                    bool hit = false;
                    if (lane > j && lane < lb && n1 + n2 <= MIRP_MAXLOOP) {
                        const int ckl = c[(size_t)k * stride + lane];
                        if (ckl < MIRP_INF)
                            hit = cij == ckl + e_intloop(P, n1, n2, pair_type(sa[k + 1], sb[lane + 1]), t2, sa[k + 2], sb[lane], si, sq);
                    }
                    const unsigned long long hits = __ballot(hit);
                    if (hits) { nk = k; nl = __ffsll((unsigned long long)hits) - 1; break; }
                }
                if (nk < 0) break;
                i = nk;
                j = nl;
            }
        }
        if (lane == 0) { out_mfe[q] = f_min < 0 ? f_min : 0; if (out_ma) { out_ma[q] = ma; out_mb[q] = mb; } }
    }
    if (evals) {
        for (int off = 32; off > 0; off >>= 1) n_eval += __shfl_xor(n_eval, off, 64);
        if (lane == 0 && n_eval) atomicAdd(evals, n_eval);
    }
}

}  // namespace mirp

namespace {

template <class SRC>
int dx_launch(mirp_ctx* c, const SRC& src, long long n, int rows, int stride, int* d_mfe, unsigned long long* d_ma, unsigned long long* d_mb,
              unsigned long long* d_evals) {
    using namespace mirp;
    if (n <= 0) return 0;
    if (rows < 1 || rows > 64 || stride < 1 || stride > 64) return fail(c, -5, "duplex: a strand longer than 64 nt reached the kernel");
    const size_t lds = sizeof(int) * DX_WAVES * ((size_t)rows * stride + DX_AUX_INTS);
    static size_t lds_set = 0;              // per instantiation
    if (lds > lds_set) {
        HIPCHK(c, hipFuncSetAttribute((const void*)duplex_kernel<SRC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set = lds;
    }
    const long long blocks = (n + DX_WAVES - 1) / DX_WAVES;
    const long long most = (long long)c->n_cu * 8 * 4;          // a few blocks per resident slot: the jobs differ in length
    c->note_jobs_per_slot(0, n, std::min(blocks, most) * DX_WAVES);
    hipLaunchKernelGGL((duplex_kernel<SRC>), dim3((unsigned)std::min(blocks, most)), dim3(64 * DX_WAVES), lds, c->stream, src, n,
                       (const FoldParams*)c->d_params, rows, stride, d_mfe, d_ma, d_mb, d_evals);
    HIPCHK(c, hipGetLastError());
    return 0;
}

}  // namespace

int mirp_device_duplex_pairs(mirp_ctx* c, const unsigned char* d_a, const long long* d_aoff, const unsigned char* d_b, const long long* d_boff, long long n,
                             int max_la, int max_lb, int* d_mfe, unsigned long long* d_ma, unsigned long long* d_mb, unsigned long long* d_evals) {
    return dx_launch(c, mirp::DxPairs{d_a, d_aoff, d_b, d_boff}, n, max_la, max_lb, d_mfe, d_ma, d_mb, d_evals);
}

int mirp_device_duplex_perfect(mirp_ctx* c, const unsigned char* d_mcodes, const TgMirna* d_mi, long long n, int* d_mfe, unsigned long long* d_ma,
                               unsigned long long* d_mb) {
    return dx_launch(c, mirp::DxPerfect{d_mcodes, d_mi}, n, 32, 32, d_mfe, d_ma, d_mb, nullptr);
}

int mirp_device_duplex_sites(mirp_ctx* c, const DxTargets& T, bool bulge, const unsigned long long* d_keys, long long n, long long max_sites,
                             const unsigned long long* d_emitted, int* d_mfe, unsigned long long* d_ma, unsigned long long* d_mb) {
    // a <= 32 nt; b = the interval (L - 1 .. L + 1 bases) and two flanks: <= 35
    if (bulge) return dx_launch(c, mirp::DxSites<true>{T, d_keys, n, max_sites, d_emitted}, n, 32, 35, d_mfe, d_ma, d_mb, nullptr);
    return dx_launch(c, mirp::DxSites<false>{T, d_keys, n, max_sites, d_emitted}, n, 32, 34, d_mfe, d_ma, d_mb, nullptr);
}

// Device side of the shuffle test of precursor MFEs (mirp_randfold, mirp_shuffle_batch; mirp_randfold.cpp), with the definitions of DESIGN.md §20.
//
// Jobs: the sequences of a call stand in an order (perm), every sequence has `jps` consecutive jobs, job j = (qi, local) = (j / jps, j % jps).  With
// has_native, local 0 is the sequence itself and local l > 0 its shuffle k = k_first + l - 1; without, local l is shuffle k_first + l.  All jobs of a
// sequence have its length, so job j's row starts at cum[qi] * jps + local * len in the job space and a pass [j0, j0 + n_jobs) is one contiguous
// piece of it: the rows (ACGUN bytes) and the offsets go straight into the buffers the fold reads.
//
//   shuffle  rf_shuffle_kernel<DI>: one lane per job.  The row lives in the output buffer and is permuted in place; the dinucleotide shuffle keeps
//            its five successor lists in the job's row of a slab of the same layout (n - 1 entries) and the per-letter counts, starts, tree edges and
//            read positions as five 12-bit fields of one 64-bit register each (n <= 3,000 < 4,096): no LDS, no private memory, and the data-dependent
//            loop of the tree walk is a plain loop of one lane.  The removed tree edge is not moved: positions of a list are read through
//            v -> v + (v >= removed), and the removed entry is read last.
//   stats    rf_stats_kernel: one lane per folded job; the shuffles of a wave are reduced per sequence (the wave's distinct sequences one after the
//            other, as wave_atomic.h does) and the leader adds le / min / S / Q to the sequence's record with one atomic each.  Integer sums: the
//            records do not depend on how the jobs fall into passes and waves.  The native job comes first in its sequence, so its MFE is in this
//            pass or already in the record.
#include <hip/hip_runtime.h>
#include <climits>
#include "mirp_ctx.h"

namespace mirp {

#define RF_G 0x9E3779B97F4A7C15ull

__device__ __forceinline__ unsigned long long rf_mix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the draws of one (seed, q, k), consumed in order
struct RfDraws {
    unsigned long long x;
    __device__ __forceinline__ RfDraws(unsigned long long seed, unsigned long long q, unsigned long long k) : x(rf_mix64(rf_mix64(seed ^ (RF_G * (q + 1))) + k)) {}
    __device__ __forceinline__ unsigned below(unsigned m) {
        x += RF_G;
        return (unsigned)(((rf_mix64(x) >> 32) * (unsigned long long)m) >> 32);
    }
};

__device__ __forceinline__ unsigned char rf_letter(unsigned c) { return (unsigned char)(0x4E55474341ull >> (8 * c)); }      // "ACGUN"[c]
__device__ __forceinline__ unsigned rf_get(unsigned long long pack, unsigned a) { return (unsigned)(pack >> (12 * a)) & 0xfffu; }

template <bool DI>
__global__ __launch_bounds__(256) void rf_shuffle_kernel(const unsigned char* __restrict__ codes, const long long* __restrict__ offs, const int* __restrict__ perm,
                                                         const long long* __restrict__ cum, long long j0, int n_jobs, long long jps, int has_native,
                                                         long long k_first, unsigned long long seed, long long base, unsigned char* __restrict__ out,
                                                         long long* __restrict__ out_offs, unsigned char* __restrict__ slab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_jobs) return;
    const long long j = j0 + i, qi = j / jps, local = j - qi * jps;
    const int q = perm[qi];
    const long long c0 = cum[qi];
    const int n = (int)(cum[qi + 1] - c0);
    const long long row = c0 * jps + local * n - base;
    out_offs[i] = row;
    if (i == n_jobs - 1) out_offs[n_jobs] = row + n;
    const unsigned char* x = codes + offs[q];
    unsigned char* y = out + row;
    if ((has_native && local == 0) || (DI && n < 3)) {
        for (int p = 0; p < n; p++) y[p] = rf_letter(x[p]);
        return;
    }
    RfDraws d(seed, (unsigned long long)q, (unsigned long long)(k_first + local - has_native));
    if (!DI) {
        for (int p = 0; p < n; p++) y[p] = rf_letter(x[p]);
        for (int p = n - 1; p > 0; p--) {
            const unsigned r = d.below((unsigned)p + 1u);
            const unsigned char a = y[p], b = y[r];
            y[p] = b; y[r] = a;
        }
        return;
    }
    // E[a]: e[start(a) .. start(a) + cnt(a)), the successors of the letter a in sequence order
    unsigned char* e = slab + row;
    unsigned long long cnt = 0;
    for (int p = 0; p < n - 1; p++) cnt += 1ull << (12 * x[p]);
    unsigned long long start = 0;
    {
        unsigned s = 0;
        for (unsigned a = 0; a < 5; a++) { start |= (unsigned long long)s << (12 * a); s += rf_get(cnt, a); }
    }
    {
        unsigned long long pos = start;
        unsigned a = x[0];
        for (int p = 1; p < n; p++) {
            const unsigned b = x[p];
            e[rf_get(pos, a)] = (unsigned char)b;
            pos += 1ull << (12 * a);
            a = b;
        }
    }
    const unsigned f = x[n - 1];
    // the last edge of every letter but f: a uniform spanning tree towards f by cycle popping
    unsigned intree = 1u << f;
    unsigned long long last = 0;
    for (unsigned a = 0; a < 5; a++) {
        if (a == f || rf_get(cnt, a) == 0) continue;
        // The walk ends with probability 1 and takes some hundred steps at worst in practice (a rare exit from a long homopolymer run); the
        // step bound only keeps a lane from spinning on a device others share.  Every letter reached has successors: it is not f.
        unsigned u = a;
        for (unsigned step = 0; !((intree >> u) & 1u) && step < (1u << 26); step++) {
            const unsigned r = d.below(rf_get(cnt, u));
            last = (last & ~(0xfffull << (12 * u))) | ((unsigned long long)r << (12 * u));
            u = e[rf_get(start, u) + r];
        }
        u = a;
        for (int step = 0; !((intree >> u) & 1u) && step < 5; step++) {
            intree |= 1u << u;
            u = e[rf_get(start, u) + rf_get(last, u)];
        }
    }
    // every list shuffled, the tree edge kept out and read last
    for (unsigned a = 0; a < 5; a++) {
        const unsigned la = rf_get(cnt, a);
        if (la == 0) continue;
        const unsigned L = a == f ? 0xffffu : rf_get(last, a), m = a == f ? la : la - 1;
        unsigned char* ea = e + rf_get(start, a);
        for (unsigned p = m; p-- > 1;) {
            const unsigned r = d.below(p + 1u);
            const unsigned pp = p + (p >= L), pr = r + (r >= L);
            const unsigned char s = ea[pp], t = ea[pr];
            ea[pp] = t; ea[pr] = s;
        }
    }
    unsigned long long ptr = 0;
    unsigned cur = x[0];
    y[0] = rf_letter(cur);
    for (int p = 1; p < n; p++) {
        const unsigned r = rf_get(ptr, cur), la = rf_get(cnt, cur), L = cur == f ? 0xffffu : rf_get(last, cur);
        ptr += 1ull << (12 * cur);
        const unsigned v = (cur != f && r + 1 == la) ? L : r + (r >= L);
        const unsigned at = min(rf_get(start, cur) + v, (unsigned)n - 2u);          // (an Euler path never leaves its list; the bound keeps a lane inside its row whatever it read)
        cur = e[at];
        y[p] = rf_letter(cur);
    }
}

__global__ __launch_bounds__(256) void rf_stats_kernel(const int* __restrict__ mfe, const int* __restrict__ status, long long j0, int n_jobs, long long jps,
                                                       const int* __restrict__ perm, MirpRandfoldRec* __restrict__ rec, int* __restrict__ bad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n_jobs;
    const int lane = threadIdx.x & 63;
    int q = -1, m = 0, nat = 0;
    bool todo = false;
    if (valid) {
        const long long j = j0 + i, qi = j / jps, local = j - qi * jps, native = qi * jps;
        q = perm[qi];
        m = mfe[i];
        if (status[i] < 0) atomicMin(bad, status[i]);
        if (local == 0) rec[q].mfe = m;
        else {
            nat = native >= j0 ? mfe[native - j0] : rec[q].mfe;          // the native job of an earlier pass: written by that pass's launch
            todo = true;
        }
    }
    while (true) {
        const unsigned long long pending = __ballot(todo);
        if (!pending) break;
        const int leader = __ffsll((long long)pending) - 1;
        const int s = __shfl(q, leader);
        const bool mine = todo && q == s;
        const int le = __popcll(__ballot(mine && m <= nat));
        int lo = mine ? m : INT_MAX;
        long long sum = mine ? (long long)m : 0ll, sq = mine ? (long long)m * m : 0ll;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o));
            sum += __shfl_xor(sum, o);
            sq += __shfl_xor(sq, o);
        }
        if (lane == leader) {
            atomicAdd(&rec[s].le, le);
            atomicMin(&rec[s].min_mfe, lo);
            atomicAdd((unsigned long long*)&rec[s].sum, (unsigned long long)sum);
            atomicAdd((unsigned long long*)&rec[s].sum_sq, (unsigned long long)sq);
        }
        if (mine) todo = false;
    }
}

}  // namespace mirp

void mirp_device_rf_shuffle(mirp_ctx* c, const RfPlan& p, long long j0, int n_jobs, long long base, unsigned char* d_out, long long* d_out_offs,
                            unsigned char* d_slab) {
    using namespace mirp;
    const dim3 grid((unsigned)((n_jobs + 255) / 256)), block(256);
    if (p.dinucleotide)
        hipLaunchKernelGGL((rf_shuffle_kernel<true>), grid, block, 0, c->stream, p.d_codes, p.d_offs, p.d_perm, p.d_cum, j0, n_jobs, p.jps, p.has_native, p.k_first,
                           p.seed, base, d_out, d_out_offs, d_slab);
    else
        hipLaunchKernelGGL((rf_shuffle_kernel<false>), grid, block, 0, c->stream, p.d_codes, p.d_offs, p.d_perm, p.d_cum, j0, n_jobs, p.jps, p.has_native, p.k_first,
                           p.seed, base, d_out, d_out_offs, d_slab);
}

void mirp_device_rf_stats(mirp_ctx* c, const RfPlan& p, long long j0, int n_jobs, const int* d_mfe, const int* d_status, MirpRandfoldRec* d_rec, int* d_bad) {
    using namespace mirp;
    hipLaunchKernelGGL(rf_stats_kernel, dim3((unsigned)((n_jobs + 255) / 256)), dim3(256), 0, c->stream, d_mfe, d_status, j0, n_jobs, p.jps, p.d_perm, d_rec, d_bad);
}

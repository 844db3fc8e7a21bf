// Device side of the 3' tail search of the read alignment (mirp_align_reads_tailed, align --tail; DESIGN.md §12 "Tails"): the reads that the
// end-to-end pass of align_kernels.hip left without a hit are searched for a templated 5' part followed by 1 .. T non-templated bases.
//
// It runs inside the hits step of a batch (mirp_device_align_hits), between al_status_kernel and the scan of the per-read slots:
//   compact   al_tail_flag_kernel, launch_excl_scan, al_tail_gather_kernel: the reads with best < 0, not suppressed by -m, L >= M + 1.  Only these
//             cost anything from here on.
//   seeds     al_tail_seed_kernel: one exact seed per read and strand.  With T_r = min(T, L - M) and s = min(M, 16) the + seed is O[0 : s] and the
//             - seed O[T_r : T_r + s] (O = the oriented read): both lie in the templated part of every admissible tail length, so every genome
//             position is a candidate of a read and strand at most once and no hit is found twice.
//   verify    launch_excl_scan over the seed ranges; al_tail_verify_kernel takes one candidate per thread: the obligatory part (O[0 : L - T_r] on
//             +, O[T_r : L] on -) must equal the genome, inside one contig and without an ambiguous base; then the match is extended base by base
//             towards the read's 3' end for up to T_r bases, which gives the tail length t of this (maximal) hit; a candidate that reaches the
//             read's end is dropped.  Pass 0 counts per read and t; al_tail_status_kernel takes the shortest tail, applies -m, sets best / supp /
//             slots / a_tt of the read and adds the read to the file's summary table (summed per distinct row of a wave first); pass 1 (after the items are allocated) writes the stratum's
//             hits as (read << 33 | offset of the templated part << 1 | strand).
// The sort, the -k cut and the emit are those of every other hit; al_record prints the tailed forms from a_tt.
//   summary   a table of (reads, depth) per tail string, indexed by (length, letters in base 5: A C G T N), resident over the batches of a file.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "align_device.h"
#include "wave_atomic.h"

namespace mirp {

#define AL_TAIL_MAX 8
#define AL_TAIL_ROWS 488280      // 5 + 5^2 + .. + 5^8

__device__ __forceinline__ bool al_bit(const unsigned* __restrict__ bm, unsigned long long p) { return (bm[p >> 5] >> (p & 31)) & 1u; }

// reads that enter the tail search: no hit at any level, not suppressed, L >= M + 1
__global__ void al_tail_flag_kernel(const int* __restrict__ best, const int* __restrict__ supp, const long long* __restrict__ roff, long long n, int M,
                                    int* __restrict__ flag) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x)
        flag[r] = best[r] < 0 && !supp[r] && roff[r + 1] - roff[r] >= (long long)M + 1;
}
__global__ void al_tail_gather_kernel(const int* __restrict__ flag, const long long* __restrict__ scan, long long n, unsigned* __restrict__ list) {
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x)
        if (flag[r]) list[scan[r]] = (unsigned)r;
}

// seed a = 2 q + strand of searched read q: slo[a] = first SA slot, ccnt[a] = slots (0 where the seed holds a letter outside ACGT)
__global__ void al_tail_seed_kernel(AlRef R, const unsigned char* __restrict__ codes, const long long* __restrict__ roff, const unsigned* __restrict__ list,
                                    long long nq, int T, int M, long long* __restrict__ slo, int* __restrict__ ccnt, int* __restrict__ overflow) {
    for (long long a = blockIdx.x * (long long)blockDim.x + threadIdx.x; a < 2 * nq; a += (long long)gridDim.x * blockDim.x) {
        const long long r = list[a >> 1];
        const int s = (int)(a & 1);
        const unsigned char* rd = codes + roff[r];
        const int L = (int)(roff[r + 1] - roff[r]);
        const int Tr = T < L - M ? T : L - M;
        const int sl = M < 16 ? M : 16;
        const int start = s ? Tr : 0;
        unsigned key = 0;
        bool bad = false;
        for (int i = 0; i < sl; i++) {
            const unsigned b = al_oriented(rd, L, s, start + i);
            bad |= b > 3u;
            key = (key << 2) | (b & 3u);
        }
        long long lo = 0, hi = 0;
        if (!bad) al_range(R, key, sl, &lo, &hi);
        slo[a] = lo;
        const long long c = hi - lo;
        if (c > 0x7fffffffll) { atomicOr(overflow, 1); ccnt[a] = 0x7fffffff; }
        else ccnt[a] = (int)c;
    }
}

// tail length 1 .. T_r of the maximal tailed hit that candidate pos of the read's seed on `strand` stands for and *o = the offset of its templated
// part, or 0: not a hit (the obligatory part fails, or the extension reaches the read's end: an end-to-end hit)
__device__ int al_tail_check(const AlRef& R, const unsigned char* __restrict__ rd, int L, int strand, int Tr, unsigned long long pos, unsigned long long* o) {
    const int ob = L - Tr;                   // the obligatory part: O[0 : ob] on +, O[Tr : L] on -, at genome [pos, pos + ob)
    const int first = strand ? Tr : 0;
    if (pos + ob > R.total) return 0;
    if (al_any(R.amb, pos, pos + ob) || al_any(R.cst, pos + 1, pos + ob)) return 0;
    for (int i = 0; i < ob; i++)
        if (al_oriented(rd, L, strand, first + i) != al_base(R.pk, pos + i)) return 0;
    if (!strand) {
        int m = ob;
        while (m < L) {                      // the next genome base in the contig, unambiguous and equal to O[m]
            const unsigned long long g = pos + m;
            if (g >= R.total || al_bit(R.amb, g) || al_bit(R.cst, g)) break;
            if ((unsigned)rd[m] != al_base(R.pk, g)) break;
            m++;
        }
        *o = pos;
        return L - m;
    }
    int t = Tr;
    unsigned long long g = pos;              // genome position of O[t]
    while (t > 0) {                          // the genome base before g in the contig, unambiguous and equal to O[t - 1]
        if (g == 0 || al_bit(R.cst, g) || al_bit(R.amb, g - 1)) break;
        if (al_oriented(rd, L, 1, t - 1) != al_base(R.pk, g - 1)) break;
        g--;
        t--;
    }
    *o = g;
    return t;
}

// pass 0: hit counts per searched read and tail length; pass 1: the hits of the read's stratum at the read's scanned offset.  One candidate per
// thread; its seed comes from a binary search over the seed scan.
template <int PASS>
__global__ void al_tail_verify_kernel(AlRef R, const unsigned char* __restrict__ codes, const long long* __restrict__ roff, const unsigned* __restrict__ list,
                                      long long nq, const long long* __restrict__ slo, const long long* __restrict__ cscan, int T, int M,
                                      unsigned* __restrict__ lvl, const unsigned char* __restrict__ tt, const int* __restrict__ best,
                                      const long long* __restrict__ off, unsigned* __restrict__ cursor, unsigned long long* __restrict__ out) {
    const long long n_seeds = 2 * nq, total = cscan[n_seeds];
    for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < total; c += (long long)gridDim.x * blockDim.x) {
        long long a = 0, z = n_seeds;                 // last seed with cscan <= c
        while (z - a > 1) { const long long md = (a + z) >> 1; if (cscan[md] <= c) a = md; else z = md; }
        const long long q = a >> 1, r = list[q];
        const int strand = (int)(a & 1);
        const unsigned long long pos = R.sa[slo[a] + (c - cscan[a])];
        const long long rb = roff[r];
        const int L = (int)(roff[r + 1] - rb);
        const int Tr = T < L - M ? T : L - M;
        unsigned long long o = 0;
        const int t = al_tail_check(R, codes + rb, L, strand, Tr, pos, &o);
        if (t == 0) continue;
        if (PASS == 0) {
            atomicAdd(&lvl[AL_TAIL_MAX * q + t - 1], 1u);
        } else if (best[r] >= 0 && (int)tt[r] == t) {
            const unsigned slot = atomicAdd(&cursor[r], 1u);
            if ((long long)slot < off[r + 1] - off[r])            // pass 0 found the same hits: always true
                out[off[r] + slot] = ((unsigned long long)r << 33) | (o << 1) | (unsigned long long)strand;
        }
    }
}

// sum of v over the 64 lanes, added to *dst by lane 0 (every lane of the wave calls it)
__device__ __forceinline__ void al_tail_wave_add(unsigned long long* dst, unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// per searched read: the shortest tail with a hit is its stratum; more than -m hits there suppress it (supp = 1, the unaligned record stays);
// otherwise best = 0, slots = the stratum's hits, tt = the tail length, and the read joins the summary table.  counts += {tailed, suppressed}.
// A library has few distinct tails, so the rows of a wave are summed per distinct row first (cl_wave_atomic: one atomic per row and wave);
// every lane of a wave stays in the loop until the wave's last read is done.
__global__ void al_tail_status_kernel(const unsigned* __restrict__ lvl, const unsigned* __restrict__ list, long long nq, int m,
                                      const unsigned char* __restrict__ codes, const long long* __restrict__ roff, const unsigned* __restrict__ depth,
                                      int* __restrict__ best, int* __restrict__ supp, int* __restrict__ slots, unsigned char* __restrict__ tt,
                                      unsigned long long* __restrict__ hist, unsigned long long* __restrict__ counts) {
    unsigned long long cnt[2] = {0, 0};
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; __any(q < nq); q += (long long)gridDim.x * blockDim.x) {
        int t = 0;
        unsigned nb = 0;
        if (q < nq)
            for (int l = 1; l <= AL_TAIL_MAX && !t; l++)
                if (lvl[AL_TAIL_MAX * q + l - 1]) { t = l; nb = lvl[AL_TAIL_MAX * q + l - 1]; }
        long long row = -1;                                          // 2 * the read's row of the table, -1: none
        unsigned long long d = 0;
        if (t) {
            const long long r = list[q];
            if (m > 0 && nb > (unsigned)m) { supp[r] = 1; cnt[1]++; }
            else {
                best[r] = 0;
                slots[r] = nb > 0x7fffffffu ? 0x7fffffff : (int)nb;
                tt[r] = (unsigned char)t;
                cnt[0]++;
                const unsigned char* rd = codes + roff[r + 1] - t;   // the last t letters as sequenced
                unsigned v = 0, base = 0, pw = 5;
                for (int i = 0; i < t; i++) v = v * 5u + rd[i];
                for (int i = 1; i < t; i++) { base += pw; pw *= 5u; }  // rows of the shorter tails come first
                row = 2 * (long long)(base + v);
                d = depth[r];
            }
        }
        cl_wave_atomic<0>(hist, row, 1ull);
        cl_wave_atomic<0>(hist + 1, row, d);
    }
    for (int i = 0; i < 2; i++) al_tail_wave_add(&counts[i], cnt[i]);
}

}  // namespace mirp

static inline int al_tail_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

static mirp::AlRef al_tail_ref(const mirp_ctx* c) {
    return mirp::AlRef{(const unsigned*)c->a_pk.p, (const unsigned*)c->a_amb.p, (const unsigned*)c->a_cst.p, (const unsigned*)c->a_sa.p,
                       (const long long*)c->a_bkt.p, (unsigned long long)c->a_total};
}

// After al_status_kernel of the uploaded batch of n reads (a_best, a_supp, a_slots set; a_depth uploaded; the summary table allocated): compaction,
// seeds, pass 0 and the strata.  Leaves a_tail_nq / a_tail_tc and the seeds for mirp_device_align_tail_hits; a_small[8..9] += {tailed, suppressed}.
int mirp_device_align_tail_strata(mirp_ctx* c, long long n, const MirpAlignTailOpts& o, int m) {
    using namespace mirp;
    hipStream_t st = c->stream;
    c->a_tail_nq = c->a_tail_tc = 0;
    if (n <= 0) return 0;
    if (c->a_tt.ensure((size_t)n)) return fail(c, -6, "device allocation failed (align: tails)");
    HIPCHK(c, hipMemsetAsync(c->a_tt.p, 0, (size_t)n, st));
    const unsigned char* d_codes = (const unsigned char*)c->a_codes.p;
    const long long* d_roff = (const long long*)c->a_roff.p;
    int* d_flag = (int*)c->a_rcnt.p;                    // the seed counts of the end-to-end pass and their scan are done with
    long long* d_fscan = (long long*)c->a_rscan.p;
    const int g = al_tail_grid(n);
    hipLaunchKernelGGL(al_tail_flag_kernel, dim3(g), dim3(256), 0, st, (const int*)c->a_best.p, (const int*)c->a_supp.p, d_roff, n, o.min_templated, d_flag);
    launch_excl_scan(st, d_flag, d_fscan, n);
    long long nq = 0;
    HIPCHK(c, hipMemcpyAsync(&nq, d_fscan + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (nq == 0) return 0;
    if (c->a_tlist.ensure(4 * (size_t)nq) || c->a_tslo.ensure(16 * (size_t)nq) || c->a_tccnt.ensure(8 * (size_t)nq) || c->a_tcscan.ensure(8 * (size_t)(2 * nq + 1)) ||
        c->a_tlvl.ensure(4 * (size_t)AL_TAIL_MAX * (size_t)nq))
        return fail(c, -6, "device allocation failed (align: tails)");
    unsigned* d_list = (unsigned*)c->a_tlist.p;
    hipLaunchKernelGGL(al_tail_gather_kernel, dim3(g), dim3(256), 0, st, (const int*)d_flag, (const long long*)d_fscan, n, d_list);
    const AlRef R = al_tail_ref(c);
    unsigned long long* d_small = (unsigned long long*)c->a_small.p;
    hipLaunchKernelGGL(al_tail_seed_kernel, dim3(al_tail_grid(2 * nq)), dim3(256), 0, st, R, d_codes, d_roff, (const unsigned*)d_list, nq, o.max_tail,
                       o.min_templated, (long long*)c->a_tslo.p, (int*)c->a_tccnt.p, (int*)(d_small + 4));
    launch_excl_scan(st, (const int*)c->a_tccnt.p, (long long*)c->a_tcscan.p, 2 * nq);
    unsigned long long ovf = 0;
    long long TC = 0;
    HIPCHK(c, hipMemcpyAsync(&ovf, d_small + 4, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&TC, (const long long*)c->a_tcscan.p + 2 * nq, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (ovf) return fail(c, -5, "a seed matches 2^31 or more index positions");
    HIPCHK(c, hipMemsetAsync(c->a_tlvl.p, 0, 4 * (size_t)AL_TAIL_MAX * (size_t)nq, st));
    if (TC > 0)
        hipLaunchKernelGGL(al_tail_verify_kernel<0>, dim3(al_tail_grid(TC)), dim3(256), 0, st, R, d_codes, d_roff, (const unsigned*)d_list, nq,
                           (const long long*)c->a_tslo.p, (const long long*)c->a_tcscan.p, o.max_tail, o.min_templated, (unsigned*)c->a_tlvl.p,
                           (const unsigned char*)nullptr, (const int*)nullptr, (const long long*)nullptr, (unsigned*)nullptr, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(al_tail_status_kernel, dim3(al_tail_grid(nq)), dim3(256), 0, st, (const unsigned*)c->a_tlvl.p, (const unsigned*)d_list, nq, m, d_codes,
                       d_roff, (const unsigned*)c->a_depth.p, (int*)c->a_best.p, (int*)c->a_supp.p, (int*)c->a_slots.p, (unsigned char*)c->a_tt.p,
                       (unsigned long long*)c->a_thist.p, d_small + 8);
    HIPCHK(c, hipStreamSynchronize(st));                 // so that the caller's clock charges these kernels to the tail pass
    HIPCHK(c, hipGetLastError());
    c->a_tail_nq = nq;
    c->a_tail_tc = TC;
    return 0;
}

// After the per-read offsets are scanned and a_items is allocated: the hits of every tailed read's stratum go to its items.
int mirp_device_align_tail_hits(mirp_ctx* c, const MirpAlignTailOpts& o) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long nq = c->a_tail_nq, TC = c->a_tail_tc;
    if (nq == 0 || TC == 0) return 0;
    hipLaunchKernelGGL(al_tail_verify_kernel<1>, dim3(al_tail_grid(TC)), dim3(256), 0, st, al_tail_ref(c), (const unsigned char*)c->a_codes.p,
                       (const long long*)c->a_roff.p, (const unsigned*)c->a_tlist.p, nq, (const long long*)c->a_tslo.p, (const long long*)c->a_tcscan.p,
                       o.max_tail, o.min_templated, (unsigned*)nullptr, (const unsigned char*)c->a_tt.p, (const int*)c->a_best.p,
                       (const long long*)c->a_off.p, (unsigned*)c->a_cursor.p, (unsigned long long*)c->a_items.p);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int mirp_device_align_tail_clear(mirp_ctx* c) {
    if (c->a_thist.ensure(16 * (size_t)AL_TAIL_ROWS)) return fail(c, -6, "device allocation failed (align: tail summary)");
    HIPCHK(c, hipMemsetAsync(c->a_thist.p, 0, 16 * (size_t)AL_TAIL_ROWS, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int mirp_device_align_tail_rows(mirp_ctx* c, std::vector<MirpTailRow>& rows) {
    std::vector<unsigned long long> h;
    try { h.resize(2 * (size_t)AL_TAIL_ROWS); } catch (...) { return fail(c, -7, "host allocation failed (align: tail summary)"); }
    HIPCHK(c, hipMemcpyAsync(h.data(), c->a_thist.p, 16 * (size_t)AL_TAIL_ROWS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rows.clear();
    size_t base = 0, count = 5;
    for (int t = 1; t <= AL_TAIL_MAX; t++, base += count, count *= 5)
        for (size_t v = 0; v < count; v++) {
            if (!h[2 * (base + v)]) continue;
            std::string s((size_t)t, 'A');
            size_t x = v;
            for (int i = t - 1; i >= 0; i--, x /= 5) s[(size_t)i] = "ACGTN"[x % 5];
            rows.push_back(MirpTailRow{s, h[2 * (base + v)], h[2 * (base + v) + 1]});
        }
    return 0;
}

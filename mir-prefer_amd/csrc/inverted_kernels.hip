// Device side of the inverted-repeat search (mirp_inverted_scan, mirp_inverted.cpp), with the semantics of DESIGN.md §30.  Integer arithmetic
// only; every result is a function of the contig and the options.
//
// Rows: the contigs stand in one array of rows, each contig from a multiple of 16 and followed by at least one padding row; a row is a left-arm
// position i.  Codes: A C G T = 0..3, anything else and the padding 4; 16 codes of 4 bits to a 64-bit word.  dmax(i) = min(D - 1, last row of
// i's contig - i) is the largest d = j - i of a cell of row i; a cell beyond it (another contig, the padding) feeds only cells beyond it, so it
// is computed like any other and merely kept out of the row's key.
//
//   scan   iv_scan_kernel: the level form, H_d[i] from H_{d-2}[i+1], H_{d-1}[i+1] and H_{d-1}[i].  One wave per tile of IV_TILE rows.  A lane
//          holds IV_R consecutive rows of H_{d-1}, H_{d-2} and the row key in registers, so 64 lanes hold a strip of IV_STRIP rows; row i + 1 of a
//          lane's last row comes from the next lane by one cross-lane shift per level.  The wave runs the strips of its tile from right to left:
//          row 0 of a strip at every level goes through `carry` (LDS, one 16-bit value per level, read one level ahead of the write that
//          replaces it) to the last row of the strip on its left.  The rightmost strip has nobody to its right and takes 0, which spoils one
//          more row to its left per level: the ceil((D - 1) / IV_STRIP) strips past the tile are that halo, recomputed and not written.
//          16 levels make a block: base i + d of row r at level d0 + k is nibble r + k of two words loaded once per block, so every extract has
//          constant operands.  Blocks whose levels lie within dmax of every row of the strip run without a test; the others (a strip that holds
//          a contig's end, the last levels when D - 1 is no multiple of 16) test d <= dmax per cell.  Row key = score << 16 | 65535 - d under an
//          unsigned maximum: the largest score, then the smallest d.
//   cand   iv_cand_kernel: the three-part rule on the row keys; with `out` null it counts the rows at or above the threshold and the
//          candidates, otherwise it appends the candidates' keys, 32767 - score << 49 | row << 12 | d, which mirp_device_sort_u64 puts into
//          selection order.
//   trace  iv_trace_kernel: one wave per candidate redoes the recurrence on the cells i <= i' < j' <= j level by level, 64 cells at a time, H of
//          the last two levels in LDS, one direction byte per cell in global memory (0 stop, 1 diagonal, 2 left base unpaired, 3 right base
//          unpaired, the definition's preferences); then lane 0 walks inwards from (i, j) and writes the ops in that order.
//   The selection (score-ordered batches, planned by bytes with plan_passes; arms kept as disjoint intervals per contig) runs on the host.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"

namespace mirp {

#define IV_R 16
#define IV_STRIP MIRP_INVERTED_STRIP
#define IV_TILE MIRP_INVERTED_TILE
#define IV_MAXSPAN MIRP_INVERTED_MAX_SPAN
#define IV_CARRY (IV_MAXSPAN + 32)

static_assert(IV_STRIP == 64 * IV_R && IV_TILE % IV_STRIP == 0, "a strip is what one wave holds; a tile is whole strips");

struct IvScore { int a, b, g; };                                     // match, mismatch, gap
struct IvJob { long long row, dir_off, ops_off; int m, pad; };       // first row, first direction byte, first op, bases i .. j
struct IvTrace { int score, left_len, right_len, n_eq, n_x, n_gap, n_ops, pad; };   // left_len: left_end - i + 1; right_len: j - right_start + 1

// one level d = d0 + k: P = H_{d-1}, Q = H_{d-2} -> Q = H_d
template <bool CHECK>
__device__ __forceinline__ void iv_level(const int (&P)[IV_R], int (&Q)[IV_R], unsigned (&key)[IV_R], const unsigned (&comp)[IV_R], const int (&dmax)[IV_R],
                                         const unsigned (&w)[4], const int k, const int d, int& nb1, int& nb2, unsigned short* carry, const int lane,
                                         const IvScore S) {
    const int ahead = carry[d];          // H_d of row 0 of the strip to the right
    int pm[IV_R + 1];
#pragma unroll
    for (int r = 0; r < IV_R; r++) pm[r] = P[r] - S.g;
    pm[IV_R] = nb1 - S.g;
    const unsigned low = 65535u - (unsigned)d;
#pragma unroll
    for (int r = 0; r < IV_R; r++) {
        const int nib = r + k;
        const unsigned code = (w[nib >> 3] >> (4 * (nib & 7))) & 15u;
        const int s = code == comp[r] ? S.a : -S.b;
        const int q = r + 1 < IV_R ? Q[(r + 1) & (IV_R - 1)] : nb2;
        const int h = max(max(q + s, pm[r]), max(pm[r + 1], 0));
        Q[r] = h;
        const unsigned hk = CHECK ? (d <= dmax[r] ? (unsigned)h : 0u) : (unsigned)h;
        key[r] = max(key[r], (hk << 16) | low);
    }
    int t = __shfl_down(Q[0], 1);
    if (lane == 63) t = ahead;
    if (lane == 0) carry[d] = (unsigned short)Q[0];
    nb2 = nb1;
    nb1 = t;
}

// the 16 levels d0 .. d0 + 15: X = H_{d0-1}, Y = H_{d0-2} -> X = H_{d0+15}, Y = H_{d0+14}; lo: the word that holds the base of the lane's row 0 at
// d0, hi: the word after it
template <bool CHECK>
__device__ __forceinline__ void iv_block(int (&X)[IV_R], int (&Y)[IV_R], unsigned (&key)[IV_R], const unsigned (&comp)[IV_R], const int (&dmax)[IV_R],
                                         const unsigned long long lo, const unsigned long long hi, const int d0, int& nb1, int& nb2, unsigned short* carry,
                                         const int lane, const IvScore S) {
    const unsigned w[4] = {(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        iv_level<CHECK>(X, Y, key, comp, dmax, w, k, d0 + k, nb1, nb2, carry, lane, S);
        iv_level<CHECK>(Y, X, key, comp, dmax, w, k + 1, d0 + k + 1, nb1, nb2, carry, lane, S);
    }
}

// blockIdx.x: tile tile0 + blockIdx.x.  words: readable up to row `rows` + IV_STRIP + IV_MAXSPAN + 128.  keys[row] for every row < rows.
__global__ __launch_bounds__(64) void iv_scan_kernel(const unsigned long long* __restrict__ words, const long long* __restrict__ pstart,
                                                     const long long* __restrict__ pend, int n_contigs, long long rows, long long tile0, int D, IvScore S,
                                                     unsigned* __restrict__ keys) {
    __shared__ unsigned short carry[IV_CARRY];
    const int lane = threadIdx.x;
    const long long base = (tile0 + blockIdx.x) * (long long)IV_TILE;
    for (int d = lane; d < IV_CARRY; d += 64) carry[d] = 0;
    __syncthreads();
    const int n_strips = IV_TILE / IV_STRIP + (D - 1 + IV_STRIP - 1) / IV_STRIP;
    const long long s_rows = (rows - 1 - base) / IV_STRIP;          // the strips past the last row are skipped
    const int s_first = s_rows < n_strips - 1 ? (int)s_rows : n_strips - 1;
    for (int s = s_first; s >= 0; s--) {
        const long long row0 = base + (long long)s * IV_STRIP + IV_R * lane;          // a multiple of 16: within one contig and its padding
        int last = -1;                                                                  // rows from row0 to the last base of its contig, - 1
        if (row0 < rows) {
            int lo = 0, hi = n_contigs - 1;                                             // the last contig that starts at or before row0
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pstart[mid] <= row0) lo = mid; else hi = mid - 1;
            }
            const long long to_end = pend[lo] - 1 - row0;
            last = to_end < IV_MAXSPAN + IV_R ? (int)to_end : IV_MAXSPAN + IV_R;
        }
        int dmax[IV_R];
        unsigned comp[IV_R], key[IV_R];
        int X[IV_R], Y[IV_R];
        const unsigned long long own = words[row0 >> 4];
        int lo_d = IV_MAXSPAN, hi_d = 0;
#pragma unroll
        for (int r = 0; r < IV_R; r++) {
            dmax[r] = max(0, min(D - 1, last - r));
            lo_d = min(lo_d, dmax[r]);
            hi_d = max(hi_d, dmax[r]);
            const unsigned code = (unsigned)(own >> (4 * r)) & 15u;
            comp[r] = code < 4u ? 3u - code : 15u;
            key[r] = 0;
            X[r] = 0;
            Y[r] = 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo_d = min(lo_d, __shfl_xor(lo_d, o));
            hi_d = max(hi_d, __shfl_xor(hi_d, o));
        }
        lo_d = __builtin_amdgcn_readfirstlane(lo_d);          // (the same in every lane: says so to the compiler, the level loops are scalar)
        hi_d = __builtin_amdgcn_readfirstlane(hi_d);
        int nb1 = 0, nb2 = 0, d0 = 0;
        // a block needs one word more than the block before it: that word is loaded a block ahead of its use
        const unsigned long long* wp = words + (row0 >> 4) + 2;
        unsigned long long w_lo = own, w_hi = wp[-1], w_next = wp[0];
        for (; d0 + 15 <= lo_d; d0 += 16) {
            const unsigned long long w_new = wp[(d0 >> 4) + 1];
            iv_block<false>(X, Y, key, comp, dmax, w_lo, w_hi, d0, nb1, nb2, carry, lane, S);
            w_lo = w_hi; w_hi = w_next; w_next = w_new;
        }
        for (; d0 <= hi_d; d0 += 16) {
            const unsigned long long w_new = wp[(d0 >> 4) + 1];
            iv_block<true>(X, Y, key, comp, dmax, w_lo, w_hi, d0, nb1, nb2, carry, lane, S);
            w_lo = w_hi; w_hi = w_next; w_next = w_new;
        }
        for (int d = d0 + lane; d < IV_CARRY; d += 64) carry[d] = 0;          // the levels this strip did not run hold 0 for the strip on its left
        __syncthreads();
        if (s < IV_TILE / IV_STRIP && row0 < rows) {
            uint4* dst = (uint4*)(keys + row0);
#pragma unroll
            for (int v = 0; v < IV_R / 4; v++) dst[v] = make_uint4(key[4 * v], key[4 * v + 1], key[4 * v + 2], key[4 * v + 3]);
        }
    }
}

__device__ __forceinline__ void iv_decode(unsigned key, int& score, int& d) {
    score = (int)(key >> 16);
    d = score ? 65535 - (int)(key & 0xffffu) : 0;
}

// counters[0] += rows with r >= min_score, counters[1] += candidates (with `out` null), counters[2] += candidates appended
__global__ void iv_cand_kernel(const unsigned* __restrict__ keys, long long rows, int min_score, unsigned long long* __restrict__ out, unsigned long long cap,
                               unsigned long long* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    for (long long at = blockIdx.x * (long long)blockDim.x; at < rows; at += (long long)gridDim.x * blockDim.x) {
        const long long i = at + threadIdx.x;
        bool above = false, cand = false;
        int sc = 0, d = 0;
        if (i < rows) {
            iv_decode(keys[i], sc, d);
            above = sc >= min_score;
        }
        if (above) {          // a row next to a contig's end has a padding row beyond it, whose key holds score 0
            int sl = 0, dl = 0, sr = 0, dr = 0;
            if (i > 0) iv_decode(keys[i - 1], sl, dl);
            if (i + 1 < rows) iv_decode(keys[i + 1], sr, dr);
            const bool continued = sl > sc && (dl - d == 1 || dl - d == 2);
            const bool decline = sr > sc && (d - dr == 1 || d - dr == 2);
            cand = !continued && !decline;
        }
        const unsigned long long ba = __ballot(above), bc = __ballot(cand);
        if (!out) {
            if (lane == 0 && ba) atomicAdd(&counters[0], (unsigned long long)__popcll(ba));
            if (lane == 0 && bc) atomicAdd(&counters[1], (unsigned long long)__popcll(bc));
        } else if (bc) {
            unsigned long long first = 0;
            if (lane == 0) first = atomicAdd(&counters[2], (unsigned long long)__popcll(bc));
            first = __shfl(first, 0);
            const unsigned long long slot = first + (unsigned long long)__popcll(bc & ((1ull << lane) - 1ull));
            if (cand && slot < cap) out[slot] = ((unsigned long long)(32767 - sc) << 49) | ((unsigned long long)i << 12) | (unsigned long long)d;
        }
    }
}

__device__ __forceinline__ unsigned iv_code(const unsigned long long* __restrict__ words, long long row) {
    return (unsigned)(words[row >> 4] >> (4 * (int)(row & 15))) & 15u;
}

// one wave per candidate.  Cell (a, a + e), 0 <= a < a + e < m, stands for (i + a, i + a + e); its direction byte is dir[e * m + a].
__global__ __launch_bounds__(64) void iv_trace_kernel(const unsigned long long* __restrict__ words, const IvJob* __restrict__ jobs, IvScore S,
                                                      unsigned char* __restrict__ dir, char* __restrict__ ops, IvTrace* __restrict__ traces) {
    __shared__ int Ha[IV_MAXSPAN + 1], Hb[IV_MAXSPAN + 1];
    __shared__ unsigned char code[IV_MAXSPAN];
    const int lane = threadIdx.x;
    const IvJob job = jobs[blockIdx.x];
    const int m = job.m;
    unsigned char* Dm = dir + job.dir_off;
    for (int a = lane; a < m; a += 64) { code[a] = (unsigned char)iv_code(words, job.row + a); Ha[a] = 0; Hb[a] = 0; }
    if (lane == 0) { Ha[m] = 0; Hb[m] = 0; }
    __syncthreads();
    int* P = Ha;          // H_{e-1}
    int* Q = Hb;          // H_{e-2}, replaced by H_e
    int score = 0;
    for (int e = 1; e < m; e++) {
        const int cells = m - e;
        for (int a = lane; a < cells; a += 64) {
            const unsigned x = code[a], y = code[a + e];
            const bool pair = x < 4u && x + y == 3u;
            const int dg = Q[a + 1] + (pair ? S.a : -S.b), up = P[a + 1] - S.g, lf = P[a] - S.g;
            const int h = max(max(dg, up), max(lf, 0));
            Q[a] = h;          // (row a - 1 read Q[a] before: ascending a, and within the 64 cells every read stands before this write)
            Dm[(long long)e * m + a] = (unsigned char)(h == 0 ? 0 : h == dg ? 1 : h == up ? 2 : 3);
            if (a == 0) score = h;
        }
        __syncthreads();          // a one-wave block: makes the level visible to the lanes that read it next
        int* t = P; P = Q; Q = t;
    }
    __syncthreads();          // (and the direction bytes to lane 0)
    if (lane != 0) return;
    int a = 0, b = m - 1, n_eq = 0, n_x = 0, n_gap = 0, left_len = 0, right_len = 0;
    long long w = job.ops_off;
    while (b > a) {
        const unsigned step = Dm[(long long)(b - a) * m + a];
        if (step == 0) break;
        char op;
        if (step == 1) {
            const unsigned x = code[a], y = code[b];
            op = x < 4u && x + y == 3u ? '=' : 'X';
            if (op == '=') n_eq++; else n_x++;
            a++; b--;
            left_len = a; right_len = m - 1 - b;
        } else if (step == 2) {
            op = 'L'; n_gap++; a++;
            left_len = a;
        } else {
            op = 'R'; n_gap++; b--;
            right_len = m - 1 - b;
        }
        ops[w++] = op;
    }
    IvTrace t;
    t.score = score; t.left_len = left_len; t.right_len = right_len; t.n_eq = n_eq; t.n_x = n_x; t.n_gap = n_gap; t.n_ops = (int)(w - job.ops_off); t.pad = 0;
    traces[blockIdx.x] = t;
}

}  // namespace mirp

namespace {

const long long kIvDefaultCapacity = 1ll << 31;
const long long kIvBatch = 4096;          // candidates a traceback pass looks at, at most

// the arms of the accepted repeats of one contig: disjoint intervals, start -> end
typedef std::map<long long, long long> IvArms;

bool iv_hits(const IvArms& arms, long long s, long long e) {          // does [s, e] share a position with an arm?
    IvArms::const_iterator it = arms.upper_bound(e);
    if (it == arms.begin()) return false;
    --it;
    return it->second >= s;
}

}  // namespace

int mirp_device_inverted(mirp_ctx* c, const IvGenome& G, const MirpInvertedOpts& o, std::vector<MirpInvertedRec>& recs, std::vector<char>& ops,
                         std::vector<long long>& ops_off) {
    using namespace mirp;
    hipStream_t st = c->stream;
    recs.clear();
    ops.clear();
    ops_off.assign(1, 0);
    const long long rows = G.rows;
    const int nc = (int)G.pstart.size() - 1;
    if (rows >= (1ll << 37)) return fail(c, -10, "mirp_inverted_scan: more than 2^37 rows");
    const long long cap = c->iv_cap > 0 ? c->iv_cap : kIvDefaultCapacity;
    const IvScore S{o.match, o.mismatch, o.gap};
    const int D = o.max_span;

    double t = mirp::now();
    if (c->iv_words.ensure(8 * G.words.size()) || c->iv_pstart.ensure(8 * ((size_t)nc + 1)) || c->iv_pend.ensure(8 * ((size_t)nc + 1)) ||
        c->iv_keys.ensure(4 * (size_t)rows) || c->iv_small.ensure(64))
        return fail(c, -6, "mirp_inverted_scan: device allocation failed (contigs)");
    HIPCHK(c, hipMemcpyAsync(c->iv_words.p, G.words.data(), 8 * G.words.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->iv_pstart.p, G.pstart.data(), 8 * ((size_t)nc + 1), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->iv_pend.p, G.pend.data(), 8 * ((size_t)nc + 1), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->iv_sec[0] = mirp::now() - t;

    // ---- scan passes over ranges of tiles whose row keys (4 bytes a row) fit the capacity; a tile that alone exceeds it has a pass of its own
    t = mirp::now();
    const long long n_tiles = (rows + IV_TILE - 1) / IV_TILE;
    const long long per_pass = std::max<long long>(1, std::min<long long>(cap / (4ll * IV_TILE), 1ll << 20));
    const unsigned long long* d_words = (const unsigned long long*)c->iv_words.p;
    c->iv_stats[10] = n_tiles;
    for (long long t0 = 0; t0 < n_tiles; t0 += per_pass) {
        const long long n = std::min(per_pass, n_tiles - t0);
        hipLaunchKernelGGL(iv_scan_kernel, dim3((unsigned)n), dim3(64), 0, st, d_words, (const long long*)c->iv_pstart.p, (const long long*)c->iv_pend.p, nc, rows,
                           t0, D, S, (unsigned*)c->iv_keys.p);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        c->iv_stats[8]++;
    }
    c->iv_sec[1] = mirp::now() - t;

    // ---- candidates: count, append, sort into selection order
    t = mirp::now();
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((rows + 255) / 256, 16384));
    unsigned long long counters[3] = {0, 0, 0};
    unsigned long long* d_counters = (unsigned long long*)c->iv_small.p;
    HIPCHK(c, hipMemsetAsync(d_counters, 0, 24, st));
    hipLaunchKernelGGL(iv_cand_kernel, dim3(grid), dim3(256), 0, st, (const unsigned*)c->iv_keys.p, rows, o.min_score, (unsigned long long*)nullptr, 0ull, d_counters);
    HIPCHK(c, hipMemcpyAsync(counters, d_counters, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const long long n_cand = (long long)counters[1];
    c->iv_stats[3] = (long long)counters[0];
    c->iv_stats[4] = n_cand;
    std::vector<unsigned long long> cand((size_t)n_cand);
    if (n_cand > 0) {
        if (c->iv_cand.ensure(8 * (size_t)n_cand) || c->iv_ctmp.ensure(8 * (size_t)n_cand))
            return fail(c, -6, "mirp_inverted_scan: device allocation failed (candidates)");
        hipLaunchKernelGGL(iv_cand_kernel, dim3(grid), dim3(256), 0, st, (const unsigned*)c->iv_keys.p, rows, o.min_score, (unsigned long long*)c->iv_cand.p,
                           (unsigned long long)n_cand, d_counters);
        HIPCHK(c, hipMemcpyAsync(counters, d_counters, 24, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        if ((long long)counters[2] != n_cand) return fail(c, -5, "mirp_inverted_scan: the two candidate passes disagree");
        if (int rc = mirp_device_sort_u64(c, (unsigned long long*)c->iv_cand.p, (unsigned long long*)c->iv_ctmp.p, n_cand, 0, 64)) return rc;
        HIPCHK(c, hipMemcpyAsync(cand.data(), c->iv_cand.p, 8 * (size_t)n_cand, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    c->iv_sec[2] = mirp::now() - t;
    if (n_cand == 0) return 0;

    // ---- traceback passes over score-ordered ranges of candidates whose direction bytes (m x m each) fit the capacity; a candidate whose end
    // base lies in an accepted arm by the time its pass is planned is dropped untraced
    struct Kept { MirpInvertedRec rec; long long ops_at; int n_ops; };
    std::vector<Kept> kept;
    std::vector<char> all_ops, region;
    std::vector<IvArms> arms((size_t)nc);
    std::vector<unsigned char> dropped((size_t)n_cand, 0);
    std::vector<IvJob> jobs;
    std::vector<IvTrace> traces;
    std::vector<long long> which;
    auto contig_of = [&](long long row) { return (int)(std::upper_bound(G.pstart.begin(), G.pstart.begin() + nc, row) - G.pstart.begin()) - 1; };
    auto span_of = [&](long long k) { return (long long)(cand[(size_t)k] & 4095ull) + 1; };
    auto bytes_of = [&](long long k) -> long long {
        const long long row = (long long)((cand[(size_t)k] >> 12) & ((1ull << 37) - 1)), m = span_of(k);
        const int ct = contig_of(row);
        const long long i = row - G.pstart[(size_t)ct] + 1, j = i + m - 1;
        if (iv_hits(arms[(size_t)ct], i, i) || iv_hits(arms[(size_t)ct], j, j)) {
            dropped[(size_t)k] = 1;
            c->iv_stats[6]++;
            return 0;
        }
        return std::min(m * m, cap);
    };
    double sec_down = 0;
    auto trace_pass = [&](long long ka, long long klast, long long) -> int {
        jobs.clear();
        which.clear();
        long long dir_at = 0, ops_at = 0;
        for (long long k = ka; k <= klast; k++) {
            if (dropped[(size_t)k]) continue;
            const long long m = span_of(k);
            jobs.push_back(IvJob{(long long)((cand[(size_t)k] >> 12) & ((1ull << 37) - 1)), dir_at, ops_at, (int)m, 0});
            which.push_back(k);
            dir_at += m * m;
            ops_at += m;
        }
        const size_t n = jobs.size();
        if (c->iv_jobs.ensure(sizeof(IvJob) * n) || c->iv_recs.ensure(sizeof(IvTrace) * n) || c->iv_dir.ensure((size_t)dir_at + 16) || c->iv_ops.ensure((size_t)ops_at + 16))
            return fail(c, -6, "mirp_inverted_scan: device allocation failed (a traceback pass)");
        HIPCHK(c, hipMemcpyAsync(c->iv_jobs.p, jobs.data(), sizeof(IvJob) * n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(iv_trace_kernel, dim3((unsigned)n), dim3(64), 0, st, d_words, (const IvJob*)c->iv_jobs.p, S, (unsigned char*)c->iv_dir.p, (char*)c->iv_ops.p,
                           (IvTrace*)c->iv_recs.p);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        const double t0 = mirp::now();
        traces.resize(n);
        region.resize((size_t)ops_at);
        HIPCHK(c, hipMemcpyAsync(traces.data(), c->iv_recs.p, sizeof(IvTrace) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(region.data(), c->iv_ops.p, (size_t)ops_at, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        sec_down += mirp::now() - t0;
        c->iv_stats[5] += (long long)n;
        c->iv_stats[9]++;
        for (size_t q = 0; q < n; q++) {
            const IvTrace& tr = traces[q];
            const IvJob& jb = jobs[q];
            const int score = 32767 - (int)(cand[(size_t)which[q]] >> 49);
            if (tr.score != score || tr.n_ops < 1 || tr.n_ops >= jb.m || tr.n_ops != tr.n_eq + tr.n_x + tr.n_gap || tr.left_len < 1 || tr.right_len < 1 ||
                tr.left_len + tr.right_len > jb.m)
                return fail(c, -5, "mirp_inverted_scan: a traceback disagrees with the row scan");
            const int ct = contig_of(jb.row);
            const long long i = jb.row - G.pstart[(size_t)ct] + 1, j = i + jb.m - 1;
            const long long le = i + tr.left_len - 1, rs = j - tr.right_len + 1;
            IvArms& A = arms[(size_t)ct];
            if (iv_hits(A, i, le) || iv_hits(A, rs, j)) continue;
            A[i] = le;
            A[rs] = j;
            Kept kp;
            kp.rec = MirpInvertedRec{ct, score, i, le, rs, j, tr.n_eq, tr.n_x, tr.n_gap, 0};
            kp.ops_at = (long long)all_ops.size();
            kp.n_ops = tr.n_ops;
            all_ops.insert(all_ops.end(), region.begin() + jb.ops_off, region.begin() + jb.ops_off + tr.n_ops);
            kept.push_back(kp);
        }
        return 0;
    };
    auto no_range = [&](long long, unsigned long long, unsigned long long, long long*) -> int { return fail(c, -5, "mirp_inverted_scan: pass plan"); };
    t = mirp::now();
    if (int rc = plan_passes(n_cand, bytes_of, cap, 1, trace_pass, no_range, kIvBatch)) return rc;
    c->iv_sec[3] = mirp::now() - t - sec_down;
    c->iv_sec[4] = sec_down;

    std::sort(kept.begin(), kept.end(), [](const Kept& x, const Kept& y) {
        if (x.rec.contig != y.rec.contig) return x.rec.contig < y.rec.contig;
        if (x.rec.left_start != y.rec.left_start) return x.rec.left_start < y.rec.left_start;
        return x.rec.right_end < y.rec.right_end;
    });
    c->iv_stats[7] = (long long)kept.size();
    for (const Kept& kp : kept) {
        recs.push_back(kp.rec);
        ops.insert(ops.end(), all_ops.begin() + kp.ops_at, all_ops.begin() + kp.ops_at + kp.n_ops);
        ops_off.push_back((long long)ops.size());
    }
    return 0;
}

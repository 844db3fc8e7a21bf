// Device side of the search for natural antisense transcripts (mirp_nats_scan, mirp_nats.cpp), with the semantics of DESIGN.md §36: seed, join,
// banded extension.  Integer arithmetic only; every result is a function of the transcripts and the options.
//
// Codes: the transcripts stand in one array of 4-bit codes, A C G T = 0..3 and 4 for every other letter and the padding; a second array holds
// their reverse complements (B') at the same places, with 5 for every other letter and the padding, so that a code of one array equals a code of
// the other only where both are known.  Every transcript starts at a multiple of 16 nibbles and has MIRP_NATS_GAP padding nibbles on either side.
//
//   keys    nt_keys_kernel: per position x the k-mer code v of A[x .. x+k-1] as a record (v << 1, transcript, x) and the code of its reverse
//           complement as (rc(v) << 1 | 1, transcript, x); a k-mer with a code above 3 (an unknown letter, the padding past the end) is left out.
//           After mirp_device_sort_hashes the forward records of a value stand before its reverse records, which are the places where B' holds it.
//   runs    nt_head_kernel / nt_start_kernel: heads of the sub-runs (value, side), their exclusive scan and the sub-runs' starts: f(v) and
//           f(rc(v)) are the lengths of two neighbouring sub-runs.
//   join    nt_join_kernel: a thread per forward record walks the reverse records of its value, a < b only.  Without `out` it adds the hits to
//           the counter of its transcript a (what plan_passes packs into passes) and counts the ignored values; with `out` it appends the keys
//           a << 38 | b << 13 | q of the transcripts a0 .. a1.  The shifted diagonal of a hit is e = x + p + k - 3 for the forward positions x in
//           A and p in B: the length of B drops out.
//   cand    nt_cand_kernel: run lengths of the sorted keys are the candidates' seeds.
//   scan    nt_scan_kernel<R, LANES>: the hot path, see there.
//   trace   nt_trace_kernel: one wave per candidate at or above the threshold redoes the band up to the end cell, anti-diagonal by
//           anti-diagonal with the latest H of every diagonal in LDS, one direction byte per band cell in global memory (0 stop, 1 diagonal,
//           2 from (i-1, j), 3 from (i, j-1): the definition's preferences); then lane 0 walks back from the end cell and writes the ops from the
//           end of its slot downwards, so that they stand in A's 5'->3' order.
//   The passes (plan_passes), the order of the jobs, the selection and the counters run on the host, below.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"

namespace mirp {

typedef unsigned long long u64;

struct NtScore { int a, b, g; };          // match, mismatch, gap
// one candidate of the band scan: a_at / b_at = nibble of A_1 / B'_1; lane l, register r, iteration k hold the cell of diagonal d = l R + r:
// i = i0 + l R/2 + ceil(r / 2) + k, j = j0 - l R/2 - floor(r / 2) + k; `blocks` blocks of 16 iterations
struct NtJob { long long a_at, b_at; int i0, j0, blocks, n, m, pad; };
struct NtBest { int score, i, j, pad; };
// one traceback: diagonals d = 0 .. w3 - 1 stand for i - j = delta0 + d; anti-diagonals t0 .. i_end + j_end
struct NtTraceJob { long long a_at, b_at, dir_off, ops_off; int delta0, t0, i_end, j_end, w3, pad; };
struct NtTrace { int score, i_start, j_start, n_eq, n_x, n_gap, n_ops, pad; };

__device__ __forceinline__ unsigned nt_nib(const u64* __restrict__ w, long long at) { return (unsigned)(w[at >> 4] >> (4 * (int)(at & 15))) & 15u; }

// counters[0] += records appended (two per k-mer without an unknown letter)
__global__ void nt_keys_kernel(const u64* __restrict__ A, const int* __restrict__ wseq, const long long* __restrict__ pos, long long n_nib, int k,
                               MirpHashRec* __restrict__ out, u64 cap, u64* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    for (long long at = blockIdx.x * (long long)blockDim.x; at < n_nib; at += (long long)gridDim.x * blockDim.x) {
        const long long g = at + threadIdx.x;
        bool ok = false;
        u64 v = 0, rc = 0;
        int s = -1;
        if (g < n_nib) s = wseq[g >> 4];
        if (s >= 0) {
            unsigned bad = 0;
            for (int j = 0; j < k; j++) {          // (the padding behind the last base holds 4: a k-mer that runs past the end is left out by its codes)
                const unsigned cd = nt_nib(A, g + j);
                bad |= cd >> 2;
                v = (v << 2) | (cd & 3u);
                rc |= (u64)(3u - (cd & 3u)) << (2 * j);
            }
            ok = bad == 0;
        }
        const u64 b = __ballot(ok);
        if (!b) continue;
        u64 first = 0;
        if (lane == __ffsll((long long)b) - 1) first = atomicAdd(&counters[0], 2ull * (u64)__popcll(b));
        first = __shfl(first, __ffsll((long long)b) - 1);
        if (ok) {
            const u64 slot = first + 2ull * (u64)__popcll(b & ((1ull << lane) - 1ull));
            if (slot + 1 < cap) {
                const unsigned x = (unsigned)(g - pos[s]) + 1u;
                MirpHashRec f, r;
                f.hash = v << 1; f.idx = (unsigned)s; f.pad = x;
                r.hash = (rc << 1) | 1ull; r.idx = (unsigned)s; r.pad = x;
                out[slot] = f;
                out[slot + 1] = r;
            }
        }
    }
}

__global__ void nt_head_kernel(const MirpHashRec* __restrict__ recs, long long n, int* __restrict__ flag) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        flag[i] = (i == 0 || recs[i].hash != recs[i - 1].hash) ? 1 : 0;
}

// starts[u] = first record of sub-run u; starts[U] = starts[U + 1] = n
__global__ void nt_start_kernel(const int* __restrict__ flag, const long long* __restrict__ scan, long long n, long long* __restrict__ starts) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (flag[i]) starts[scan[i]] = i;
        if (i == 0) { starts[scan[n]] = n; starts[scan[n] + 1] = n; }
    }
}

// counters[1] += ignored values, counters[2] += keys appended; cnt[a] += hits of transcript a
template <bool EMIT>
__global__ void nt_join_kernel(const MirpHashRec* __restrict__ recs, long long n, const int* __restrict__ flag, const long long* __restrict__ scan,
                               const long long* __restrict__ starts, int max_occ, int k, int wshift, unsigned a0, unsigned a1, u64* __restrict__ cnt,
                               u64* __restrict__ out, u64 cap, u64* __restrict__ counters) {
    const long long n_runs = scan[n];
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const MirpHashRec r = recs[i];
        if (r.hash & 1ull) continue;
        if (EMIT && (r.idx < a0 || r.idx > a1)) continue;
        const long long u = scan[i] + flag[i] - 1;
        const long long s0 = starts[u], s1 = starts[u + 1];
        long long s2 = s1;
        if (u + 1 < n_runs && recs[s1].hash == (r.hash | 1ull)) s2 = starts[u + 2];
        const bool ignored = s1 - s0 > max_occ || s2 - s1 > max_occ;
        if (!EMIT && i == s0 && ignored) atomicAdd(&counters[1], 1ull);
        if (ignored || s2 == s1) continue;
        u64 hits = 0;
        for (long long t = s1; t < s2; t++) hits += recs[t].idx > r.idx ? 1u : 0u;
        if (!hits) continue;
        if (!EMIT) {
            atomicAdd(&cnt[r.idx], hits);
            continue;
        }
        u64 slot = atomicAdd(&counters[2], hits);
        for (long long t = s1; t < s2; t++) {
            const MirpHashRec p = recs[t];
            if (p.idx <= r.idx) continue;
            const u64 e = (u64)r.pad + (u64)p.pad + (u64)k - 3ull;
            if (slot < cap) out[slot] = ((u64)r.idx << 38) | ((u64)p.idx << 13) | (e >> wshift);
            slot++;
        }
    }
}

// counters[3] += candidates, counters[4] += kept candidates appended as (key, seeds)
__global__ void nt_cand_kernel(const u64* __restrict__ hits, long long n, int min_seeds, u64* __restrict__ out, u64 cap, u64* __restrict__ counters) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const u64 key = hits[i];
        if (i > 0 && hits[i - 1] == key) continue;
        long long len = 1;
        while (i + len < n && hits[i + len] == key) len++;
        atomicAdd(&counters[3], 1ull);
        if (len < min_seeds) continue;
        const u64 slot = atomicAdd(&counters[4], 1ull);
        if (slot < cap) { out[2 * slot] = key; out[2 * slot + 1] = (u64)len; }
    }
}

// 24 nibbles from nibble s / 4 of w0 on
__device__ __forceinline__ void nt_window(const u64 w0, const u64 w1, const u64 w2, const int s, unsigned (&out)[3]) {
    const u64 lo = s ? (w0 >> s) | (w1 << (64 - s)) : w0;
    const u64 hi = s ? (w1 >> s) | (w2 << (64 - s)) : w1;
    out[0] = (unsigned)lo;
    out[1] = (unsigned)(lo >> 32);
    out[2] = (unsigned)hi;
}

#define NT_NIB(w, x) (((w)[(x) >> 3] >> (4 * ((x) & 7))) & 15u)

// The band scan.  One wave per candidate, stepping over anti-diagonals t = i + j.  The band's 3 W diagonals d = i - j - delta0 are spread over
// LANES lanes, R consecutive ones to a lane (R even, LANES R = 3 W); h[r] is the latest H on diagonal l R + r.  On anti-diagonal t only the
// diagonals of one parity hold a cell, and that cell needs H of its own diagonal at t - 2 and of its two neighbours at t - 1, which is what the h
// of the other parity hold: an iteration renews the even registers (t) from the odd ones and then the odd registers (t + 1) from the even ones,
// every register once per cell, no cell computed that is not one.  The neighbours beyond a lane's registers come by one cross-lane move per
// parity; beyond the band they are 0.  16 iterations make a block: within it the bases of a register's cells are nibbles k + const of two
// 24-nibble windows built once per block from three words each, so every extract has constant operands.
// No test of i or j inside the loop (the padding-code argument of §25): a cell before the matrix (i < 1 or j < 1) holds 0 because the padding
// equals nothing and everything it depends on lies before the matrix too; a cell past it (i > n or j > m) feeds only cells past it and holds
// strictly less than some cell inside, so it never is the maximum.  key[r]: the running unsigned maximum of H << 12 | 4095 - (iteration mod
// 4096), i.e. the largest H of a diagonal within a segment of 4,096 iterations and the first iteration that reached it (H < 2^20: 65,535
// bases at the largest match score); at a segment's end the keys go into best[r] / bk[r], the largest H of the diagonal and its cell with the
// smallest i.  The end cell (largest H, then smallest i, then smallest j) is the maximum over the diagonals of one 64-bit key, taken once per
// candidate.  A wave serves the jobs blockIdx.x, blockIdx.x + gridDim.x, ...
// Reach: at every step some lane holds a cell of the matrix and the others lie within 3 W / 2 <= 384 of it in i and in j; the last block adds at
// most 15 iterations and a window 32 nibbles with the word loaded ahead, so no read leaves the MIRP_NATS_GAP = 1,024 padding nibbles around a
// transcript (mirp_device_nats derives i0, j0 and `blocks` from the band's first and last anti-diagonal inside the matrix).
template <int R, int LANES>
__global__ __launch_bounds__(64) void nt_scan_kernel(const u64* __restrict__ A, const u64* __restrict__ B, const NtJob* __restrict__ jobs, int n_jobs,
                                                     NtScore S, NtBest* __restrict__ out) {
    constexpr int H = R / 2;
    static_assert(R % 2 == 0 && R <= 12 && LANES <= 64, "an even number of diagonals per lane; the windows hold 15 + R / 2 + 1 nibbles");
    static_assert(MIRP_NATS_MAX_LEN * 10 < (1 << 20), "H << 12 fits 32 bits");
    const int lane = threadIdx.x;
    for (int job = blockIdx.x; job < n_jobs; job += gridDim.x) {
        const NtJob jb = jobs[job];
        const long long ai = jb.a_at + jb.i0 - 1 + lane * H;                  // nibble of A_i, i of register 0 at iteration 0
        const long long bi = jb.b_at + jb.j0 - 1 - lane * H - (H - 1);        // nibble of B'_j, the smallest j of the lane's registers at iteration 0
        const int sa = 4 * (int)(ai & 15), sb = 4 * (int)(bi & 15);
        const u64* ap = A + (ai >> 4);
        const u64* bp = B + (bi >> 4);
        u64 a0 = ap[0], a1 = ap[1], b0 = bp[0], b1 = bp[1];
        int h[R], best[R], bk[R];
        unsigned key[R];
#pragma unroll
        for (int r = 0; r < R; r++) { h[r] = 0; best[r] = 0; bk[r] = 0; key[r] = 0; }
        for (int blk = 0; blk < jb.blocks; blk++) {
            const u64 a2 = ap[blk + 2], b2 = bp[blk + 2];
            unsigned aw[3], bw[3];
            nt_window(a0, a1, a2, sa, aw);
            nt_window(b0, b1, b2, sb, bw);
#pragma unroll
            for (int kk = 0; kk < 16; kk++) {
                const unsigned low = 4095u - (unsigned)((16 * blk + kk) & 4095);
                int lf = __shfl_up(h[R - 1], 1);
                if (lane == 0) lf = 0;
#pragma unroll
                for (int r = 0; r < R; r += 2) {          // diagonal l R + r: i = .. + r / 2 + k, j = .. - r / 2 + k
                    const unsigned ca = NT_NIB(aw, kk + r / 2), cb = NT_NIB(bw, kk + H - 1 - r / 2);
                    const int dg = h[r] + (ca == cb ? S.a : -S.b);
                    const int up = (r ? h[r > 0 ? r - 1 : 0] : lf) - S.g, left = h[r + 1] - S.g;
                    const int hv = max(max(dg, max(up, left)), 0);
                    h[r] = hv;
                    key[r] = max(key[r], ((unsigned)hv << 12) | low);
                }
                int rt = __shfl_down(h[0], 1);
                if (lane >= LANES - 1) rt = 0;
#pragma unroll
                for (int r = 1; r < R; r += 2) {          // i = .. + (r + 1) / 2 + k, j = .. - (r - 1) / 2 + k
                    const unsigned ca = NT_NIB(aw, kk + (r + 1) / 2), cb = NT_NIB(bw, kk + H - 1 - (r - 1) / 2);
                    const int dg = h[r] + (ca == cb ? S.a : -S.b);
                    const int up = h[r - 1] - S.g, left = (r + 1 < R ? h[r + 1 < R ? r + 1 : 0] : rt) - S.g;
                    const int hv = max(max(dg, max(up, left)), 0);
                    h[r] = hv;
                    key[r] = max(key[r], ((unsigned)hv << 12) | low);
                }
            }
            a0 = a1; a1 = a2; b0 = b1; b1 = b2;
            if ((blk & 255) == 255 || blk + 1 == jb.blocks) {          // the end of a segment of 4,096 iterations: its keys into best / bk
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int hs = (int)(key[r] >> 12);
                    if (hs > best[r]) { best[r] = hs; bk[r] = 16 * (blk & ~255) + 4095 - (int)(key[r] & 4095u); }
                    key[r] = 0;
                }
            }
        }
        u64 top = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int i = jb.i0 + lane * H + (r + 1) / 2 + bk[r], j = jb.j0 - lane * H - r / 2 + bk[r];
            const bool in = lane < LANES && best[r] > 0 && i >= 1 && i <= jb.n && j >= 1 && j <= jb.m;
            const u64 kr = in ? ((u64)best[r] << 32) | ((u64)(65535 - i) << 16) | (u64)(65535 - j) : 0ull;
            top = kr > top ? kr : top;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(top, o);
            top = other > top ? other : top;
        }
        if (lane == 0) {
            NtBest bst;
            bst.score = (int)(top >> 32);
            bst.i = top ? 65535 - (int)((top >> 16) & 0xffffu) : 0;
            bst.j = top ? 65535 - (int)(top & 0xffffu) : 0;
            bst.pad = 0;
            out[job] = bst;
        }
    }
}

#define NT_MAX_W3 768

// one wave per job.  The direction byte of cell (i, j) is dir[dir_off + (i + j - t0) * w3 + d], d = i - j - delta0.
__global__ __launch_bounds__(64) void nt_trace_kernel(const u64* __restrict__ A, const u64* __restrict__ B, const NtTraceJob* __restrict__ jobs, NtScore S,
                                                      unsigned char* __restrict__ dir, char* __restrict__ ops, NtTrace* __restrict__ traces) {
    __shared__ int h[NT_MAX_W3 + 2];          // h[d + 1]: the latest H of diagonal d; h[0] and h[w3 + 1] lie beyond the band
    __shared__ int end_score;
    const int lane = threadIdx.x;
    const NtTraceJob jb = jobs[blockIdx.x];
    const int w3 = jb.w3, t_end = jb.i_end + jb.j_end;
    unsigned char* Dm = dir + jb.dir_off;
    for (int d = lane; d < w3 + 2; d += 64) h[d] = 0;
    if (lane == 0) end_score = 0;
    __syncthreads();
    for (int t = jb.t0; t <= t_end; t++) {
        const int par = (t + jb.delta0) & 1;
        for (int d = par + 2 * lane; d < w3; d += 128) {
            const int i = (t + jb.delta0 + d) >> 1, j = t - i;          // (t + delta0 + d is even)
            const unsigned ca = nt_nib(A, jb.a_at + i - 1), cb = nt_nib(B, jb.b_at + j - 1);
            const int dg = h[d + 1] + (ca == cb ? S.a : -S.b), up = h[d] - S.g, left = h[d + 2] - S.g;
            const int hv = max(max(dg, up), max(left, 0));
            h[d + 1] = hv;          // (the neighbours read at this step belong to the other parity: nobody writes them now)
            Dm[(long long)(t - jb.t0) * w3 + d] = (unsigned char)(hv == 0 ? 0 : hv == dg ? 1 : hv == up ? 2 : 3);
            if (i == jb.i_end && j == jb.j_end) end_score = hv;
        }
        __syncthreads();          // a one-wave block: makes the step visible to the lanes that read it next
    }
    __syncthreads();          // (and the direction bytes to lane 0)
    if (lane != 0) return;
    int i = jb.i_end, j = jb.j_end, li = i, lj = j, n_eq = 0, n_x = 0, n_gap = 0;
    long long w = jb.ops_off + t_end;
    const long long w_end = w;
    while (i >= 1 && j >= 1 && i + j >= jb.t0) {
        const int d = i - j - jb.delta0;
        if (d < 0 || d >= w3) break;
        const unsigned step = Dm[(long long)(i + j - jb.t0) * w3 + d];
        if (step == 0) break;
        li = i; lj = j;
        char op;
        if (step == 1) {
            op = nt_nib(A, jb.a_at + i - 1) == nt_nib(B, jb.b_at + j - 1) ? '=' : 'X';
            if (op == '=') n_eq++; else n_x++;
            i--; j--;
        } else if (step == 2) {
            op = 'I'; n_gap++; i--;
        } else {
            op = 'D'; n_gap++; j--;
        }
        ops[--w] = op;
    }
    NtTrace tr;
    tr.score = end_score; tr.i_start = li; tr.j_start = lj; tr.n_eq = n_eq; tr.n_x = n_x; tr.n_gap = n_gap; tr.n_ops = (int)(w_end - w); tr.pad = 0;
    traces[blockIdx.x] = tr;
}

}  // namespace mirp

namespace {

const long long kNtDefaultCapacity = 1ll << 31;
const long long kNtScanBatch = 1ll << 20;          // candidates per launch of the band scan
const long long kNtTraceBatch = 4096;              // candidates a traceback pass looks at, at most

struct NtCand { unsigned long long key; long long seeds; int a, b, q, score, i_end, j_end, t0, delta0; };

// band cells of a candidate inside the n x m matrix: the diagonals e = lo .. hi of the n + m - 1, diagonal e holding min(e + 1, p, n + m - 1 - e) cells
long long nt_diag_prefix(long long u, long long n, long long m) {          // cells of the first u diagonals
    const long long p = std::min(n, m), D = n + m - 1;
    if (u <= 0) return 0;
    if (u <= p - 1) return u * (u + 1) / 2;
    if (u <= D - (p - 1)) return (p - 1) * p / 2 + (u - (p - 1)) * p;
    const long long r = D - u;
    return n * m - r * (r + 1) / 2;
}

template <int R, int LANES>
void nt_launch_scan(hipStream_t st, unsigned grid, const unsigned long long* A, const unsigned long long* B, const mirp::NtJob* jobs, int n, mirp::NtScore S,
                    mirp::NtBest* out) {
    hipLaunchKernelGGL((mirp::nt_scan_kernel<R, LANES>), dim3(grid), dim3(64), 0, st, A, B, jobs, n, S, out);
}

}  // namespace

int mirp_device_nats(mirp_ctx* c, const NtSeqs& T, const MirpNatsOpts& o, std::vector<MirpNatsRec>& recs, std::vector<char>& ops, std::vector<long long>& ops_off) {
    using namespace mirp;
    hipStream_t st = c->stream;
    recs.clear();
    ops.clear();
    ops_off.assign(1, 0);
    const int n_seqs = (int)T.len.size();
    const long long n_words = (long long)T.fwd.size(), n_nib = 16 * n_words;
    const long long cap = c->nt_cap > 0 ? c->nt_cap : kNtDefaultCapacity;
    const NtScore S{o.match, o.mismatch, o.gap};
    const int W = o.band, k = o.seed;
    int wshift = 0;
    while ((1 << wshift) < W) wshift++;
    long long bases = 0;
    for (int s = 0; s < n_seqs; s++) bases += T.len[(size_t)s];

    // ---- upload, keys
    double t = mirp::now();
    const long long max_recs = 2 * bases;
    if (c->nt_a.ensure(8 * (size_t)n_words) || c->nt_b.ensure(8 * (size_t)n_words) || c->nt_wseq.ensure(4 * (size_t)n_words) ||
        c->nt_pos.ensure(8 * (size_t)n_seqs) || c->nt_small.ensure(64) || c->nt_recs.ensure(16 * (size_t)max_recs + 16) ||
        c->nt_rtmp.ensure(16 * (size_t)max_recs + 16) || c->nt_cnt.ensure(8 * (size_t)n_seqs))
        return fail(c, -6, "mirp_nats_scan: device allocation failed (transcripts and k-mer records)");
    const u64* d_A = (const u64*)c->nt_a.p;
    const u64* d_B = (const u64*)c->nt_b.p;
    u64* d_counters = (u64*)c->nt_small.p;
    u64 counters[5] = {0, 0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(c->nt_a.p, T.fwd.data(), 8 * (size_t)n_words, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->nt_b.p, T.rc.data(), 8 * (size_t)n_words, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->nt_wseq.p, T.wseq.data(), 4 * (size_t)n_words, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->nt_pos.p, T.pos.data(), 8 * (size_t)n_seqs, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_counters, 0, 40, st));
    HIPCHK(c, hipMemsetAsync(c->nt_cnt.p, 0, 8 * (size_t)n_seqs, st));
    auto grid_of = [](long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 16384)); };
    hipLaunchKernelGGL(nt_keys_kernel, dim3(grid_of(n_nib)), dim3(256), 0, st, d_A, (const int*)c->nt_wseq.p, (const long long*)c->nt_pos.p, n_nib, k,
                       (MirpHashRec*)c->nt_recs.p, (u64)max_recs, d_counters);
    HIPCHK(c, hipMemcpyAsync(counters, d_counters, 40, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    const long long n_recs = (long long)counters[0];
    if (n_recs > max_recs) return fail(c, -5, "mirp_nats_scan: more k-mer records than positions");
    c->nt_sec[0] = mirp::now() - t;
    if (n_recs == 0) return 0;

    // ---- sort, sub-runs
    t = mirp::now();
    MirpHashRec* d_recs = (MirpHashRec*)c->nt_recs.p;
    if (int rc = mirp_device_sort_hashes(c, d_recs, (MirpHashRec*)c->nt_rtmp.p, n_recs, 2 * k + 1)) return rc;
    if (c->nt_flag.ensure(4 * (size_t)n_recs) || c->nt_scan.ensure(8 * (size_t)(n_recs + 1)) || c->nt_starts.ensure(8 * (size_t)(n_recs + 2)))
        return fail(c, -6, "mirp_nats_scan: device allocation failed (runs)");
    int* d_flag = (int*)c->nt_flag.p;
    long long* d_scan = (long long*)c->nt_scan.p;
    long long* d_starts = (long long*)c->nt_starts.p;
    hipLaunchKernelGGL(nt_head_kernel, dim3(grid_of(n_recs)), dim3(256), 0, st, (const MirpHashRec*)d_recs, n_recs, d_flag);
    launch_excl_scan(st, d_flag, d_scan, n_recs);
    hipLaunchKernelGGL(nt_start_kernel, dim3(grid_of(n_recs)), dim3(256), 0, st, (const int*)d_flag, (const long long*)d_scan, n_recs, d_starts);
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    c->nt_sec[1] = mirp::now() - t;

    // ---- join: the hits per transcript a, then passes over ranges of a whose hits (16 bytes each) fit the capacity; a transcript that alone
    // exceeds it has a pass of its own
    t = mirp::now();
    u64* d_cnt = (u64*)c->nt_cnt.p;
    hipLaunchKernelGGL(nt_join_kernel<false>, dim3(grid_of(n_recs)), dim3(256), 0, st, (const MirpHashRec*)d_recs, n_recs, (const int*)d_flag,
                       (const long long*)d_scan, (const long long*)d_starts, o.max_occ, k, wshift, 0u, 0u, d_cnt, (u64*)nullptr, 0ull, d_counters);
    std::vector<u64> per_a((size_t)n_seqs);
    HIPCHK(c, hipMemcpyAsync(per_a.data(), d_cnt, 8 * (size_t)n_seqs, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(counters, d_counters, 40, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    c->nt_stats[3] = (long long)counters[1];
    const long long hit_cap = std::max<long long>(1, cap / 16);
    std::vector<NtCand> cands;
    std::vector<u64> pass_cands;
    auto join_pass = [&](long long a_first, long long a_last, long long) -> int {
        long long expected = 0;
        for (long long a = a_first; a <= a_last; a++) expected += (long long)per_a[(size_t)a];
        if (c->nt_hits.ensure(8 * (size_t)expected) || c->nt_htmp.ensure(8 * (size_t)expected) || c->nt_cand.ensure(16 * (size_t)expected))
            return fail(c, -6, "mirp_nats_scan: device allocation failed (a join pass)");
        HIPCHK(c, hipMemsetAsync(d_counters + 2, 0, 24, st));
        hipLaunchKernelGGL(nt_join_kernel<true>, dim3(grid_of(n_recs)), dim3(256), 0, st, (const MirpHashRec*)d_recs, n_recs, (const int*)d_flag,
                           (const long long*)d_scan, (const long long*)d_starts, o.max_occ, k, wshift, (unsigned)a_first, (unsigned)a_last, d_cnt,
                           (u64*)c->nt_hits.p, (u64)expected, d_counters);
        if (int rc = mirp_device_sort_u64(c, (u64*)c->nt_hits.p, (u64*)c->nt_htmp.p, expected, 0, 64)) return rc;
        hipLaunchKernelGGL(nt_cand_kernel, dim3(grid_of(expected)), dim3(256), 0, st, (const u64*)c->nt_hits.p, expected, o.min_seeds, (u64*)c->nt_cand.p,
                           (u64)expected, d_counters);
        u64 got[5];
        HIPCHK(c, hipMemcpyAsync(got, d_counters, 40, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        if ((long long)got[2] != expected) return fail(c, -5, "mirp_nats_scan: the two join passes disagree");
        c->nt_stats[4] += expected;
        c->nt_stats[5] += (long long)got[3];
        c->nt_stats[12]++;
        const size_t kept = (size_t)got[4];
        pass_cands.resize(2 * kept);
        if (kept) HIPCHK(c, hipMemcpy(pass_cands.data(), c->nt_cand.p, 16 * kept, hipMemcpyDeviceToHost));
        for (size_t q = 0; q < kept; q++) {
            NtCand cd;
            std::memset(&cd, 0, sizeof cd);
            cd.key = pass_cands[2 * q];
            cd.seeds = (long long)pass_cands[2 * q + 1];
            cd.a = (int)(cd.key >> 38);
            cd.b = (int)((cd.key >> 13) & ((1ull << 25) - 1));
            cd.q = (int)(cd.key & 8191ull);
            cands.push_back(cd);
        }
        return 0;
    };
    auto no_range = [&](long long, unsigned long long, unsigned long long, long long*) -> int { return fail(c, -5, "mirp_nats_scan: pass plan"); };
    auto hits_of = [&](long long a) -> long long { return std::min<long long>((long long)per_a[(size_t)a], hit_cap); };
    if (int rc = plan_passes(n_seqs, hits_of, hit_cap, 1, join_pass, no_range)) return rc;
    std::sort(cands.begin(), cands.end(), [](const NtCand& x, const NtCand& y) { return x.key < y.key; });
    const long long n_cand = (long long)cands.size();
    c->nt_stats[6] = n_cand;
    c->nt_sec[2] = mirp::now() - t;
    if (n_cand == 0) return 0;

    // ---- band scan: the jobs by falling length, so that the waves of a launch finish together; a wave serves every `grid`-th job
    t = mirp::now();
    std::vector<NtJob> jobs((size_t)n_cand);
    for (long long x = 0; x < n_cand; x++) {
        NtCand& cd = cands[(size_t)x];
        const long long n = T.len[(size_t)cd.a], m = T.len[(size_t)cd.b];
        const long long e0 = ((long long)cd.q - 1) * W, e_lo = std::max(e0, 0ll), e_hi = std::min(e0 + 3 * W - 1, n + m - 2);
        const long long dl = e_lo - (m - 1), dh = e_hi - (m - 1), delta0 = e0 - (m - 1);
        const long long t_min = 2 + (dl <= 0 && dh >= 0 ? 0 : std::min(std::llabs(dl), std::llabs(dh)));
        const long long t_max = dh < n - m ? 2 * m + dh : dl > n - m ? 2 * n - dl : n + m;
        const long long t0 = ((t_min + delta0) & 1) ? t_min - 1 : t_min;
        c->nt_stats[7] += nt_diag_prefix(e_hi + 1, n, m) - nt_diag_prefix(e_lo, n, m);
        cd.t0 = (int)t0;
        cd.delta0 = (int)delta0;
        NtJob& jb = jobs[(size_t)x];
        jb.a_at = T.pos[(size_t)cd.a];
        jb.b_at = T.pos[(size_t)cd.b];
        jb.i0 = (int)((t0 + delta0) / 2);          // (even: exact for a negative sum too)
        jb.j0 = (int)((t0 - delta0) / 2);
        jb.blocks = (int)(((t_max - t0) / 2 + 1 + 15) / 16);
        jb.n = (int)n;
        jb.m = (int)m;
        jb.pad = (int)x;
    }
    std::stable_sort(jobs.begin(), jobs.end(), [](const NtJob& x, const NtJob& y) { return x.blocks > y.blocks; });
    c->reset_jobs_per_slot(8);
    std::vector<NtBest> bests;
    for (long long x0 = 0; x0 < n_cand; x0 += kNtScanBatch) {
        const long long n = std::min(kNtScanBatch, n_cand - x0);
        if (c->nt_jobs.ensure(sizeof(NtJob) * (size_t)n) || c->nt_best.ensure(sizeof(NtBest) * (size_t)n))
            return fail(c, -6, "mirp_nats_scan: device allocation failed (the band scan)");
        HIPCHK(c, hipMemcpyAsync(c->nt_jobs.p, jobs.data() + x0, sizeof(NtJob) * (size_t)n, hipMemcpyHostToDevice, st));
        const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((n + 3) / 4, 8ll * c->n_cu));
        const NtJob* dj = (const NtJob*)c->nt_jobs.p;
        NtBest* db = (NtBest*)c->nt_best.p;
        switch (W) {
            case 16: nt_launch_scan<2, 24>(st, grid, d_A, d_B, dj, (int)n, S, db); break;
            case 32: nt_launch_scan<2, 48>(st, grid, d_A, d_B, dj, (int)n, S, db); break;
            case 64: nt_launch_scan<4, 48>(st, grid, d_A, d_B, dj, (int)n, S, db); break;
            case 128: nt_launch_scan<6, 64>(st, grid, d_A, d_B, dj, (int)n, S, db); break;
            default: nt_launch_scan<12, 64>(st, grid, d_A, d_B, dj, (int)n, S, db); break;
        }
        c->note_jobs_per_slot(8, n, grid);
        bests.resize((size_t)n);
        HIPCHK(c, hipMemcpyAsync(bests.data(), db, sizeof(NtBest) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        c->nt_stats[13]++;
        for (long long x = 0; x < n; x++) {
            NtCand& cd = cands[(size_t)jobs[(size_t)(x0 + x)].pad];
            cd.score = bests[(size_t)x].score;
            cd.i_end = bests[(size_t)x].i;
            cd.j_end = bests[(size_t)x].j;
        }
    }
    c->nt_sec[3] = mirp::now() - t;

    // ---- traceback passes over the candidates at or above the threshold, in candidate order, whose direction bytes fit the capacity
    t = mirp::now();
    std::vector<long long> above;
    for (long long x = 0; x < n_cand; x++)
        if (cands[(size_t)x].score >= o.min_score) above.push_back(x);
    c->nt_stats[8] = (long long)above.size();
    struct Kept { MirpNatsRec rec; long long ops_at; int n_ops; };
    std::vector<Kept> kept;
    std::vector<char> all_ops, region;
    std::vector<NtTraceJob> tjobs;
    std::vector<NtTrace> traces;
    auto dir_bytes = [&](long long y) -> long long {
        const NtCand& cd = cands[(size_t)above[(size_t)y]];
        return 3ll * W * ((long long)cd.i_end + cd.j_end - cd.t0 + 1);
    };
    auto trace_pass = [&](long long ya, long long ylast, long long) -> int {
        tjobs.clear();
        long long dir_at = 0, ops_at = 0;
        for (long long y = ya; y <= ylast; y++) {
            const NtCand& cd = cands[(size_t)above[(size_t)y]];
            NtTraceJob jb;
            jb.a_at = T.pos[(size_t)cd.a]; jb.b_at = T.pos[(size_t)cd.b]; jb.dir_off = dir_at; jb.ops_off = ops_at;
            jb.delta0 = cd.delta0; jb.t0 = cd.t0; jb.i_end = cd.i_end; jb.j_end = cd.j_end; jb.w3 = 3 * W; jb.pad = 0;
            tjobs.push_back(jb);
            dir_at += dir_bytes(y);
            ops_at += (long long)cd.i_end + cd.j_end;
        }
        const size_t n = tjobs.size();
        if (c->nt_tjobs.ensure(sizeof(NtTraceJob) * n) || c->nt_trec.ensure(sizeof(NtTrace) * n) || c->nt_dir.ensure((size_t)dir_at + 16) ||
            c->nt_ops.ensure((size_t)ops_at + 16))
            return fail(c, -6, "mirp_nats_scan: device allocation failed (a traceback pass)");
        HIPCHK(c, hipMemcpyAsync(c->nt_tjobs.p, tjobs.data(), sizeof(NtTraceJob) * n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(nt_trace_kernel, dim3((unsigned)n), dim3(64), 0, st, d_A, d_B, (const NtTraceJob*)c->nt_tjobs.p, S, (unsigned char*)c->nt_dir.p,
                           (char*)c->nt_ops.p, (NtTrace*)c->nt_trec.p);
        traces.resize(n);
        region.resize((size_t)ops_at);
        HIPCHK(c, hipMemcpyAsync(traces.data(), c->nt_trec.p, sizeof(NtTrace) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(region.data(), c->nt_ops.p, (size_t)ops_at, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        c->nt_stats[9] += (long long)n;
        c->nt_stats[14]++;
        for (size_t q = 0; q < n; q++) {
            const NtTrace& tr = traces[q];
            const NtTraceJob& jb = tjobs[q];
            const NtCand& cd = cands[(size_t)above[(size_t)(ya + (long long)q)]];
            if (tr.score != cd.score || tr.n_ops < 1 || tr.n_ops > jb.i_end + jb.j_end || tr.n_ops != tr.n_eq + tr.n_x + tr.n_gap || tr.i_start < 1 ||
                tr.j_start < 1 || tr.i_start > jb.i_end || tr.j_start > jb.j_end)
                return fail(c, -5, "mirp_nats_scan: a traceback disagrees with the band scan");
            if (tr.n_ops < o.min_length) continue;
            const int n_len = T.len[(size_t)cd.a], m_len = T.len[(size_t)cd.b];
            Kept kp;
            kp.rec = MirpNatsRec{cd.a, cd.b, cd.score, tr.i_start, jb.i_end, n_len, m_len + 1 - jb.j_end, m_len + 1 - tr.j_start, m_len, tr.n_eq, tr.n_x, tr.n_gap,
                                 (int)std::min<long long>(cd.seeds, 2147483647ll), cd.q};
            kp.ops_at = (long long)all_ops.size();
            kp.n_ops = tr.n_ops;
            const long long first = jb.ops_off + jb.i_end + jb.j_end - tr.n_ops;
            all_ops.insert(all_ops.end(), region.begin() + first, region.begin() + first + tr.n_ops);
            kept.push_back(kp);
        }
        return 0;
    };
    auto bytes_of = [&](long long y) -> long long { return std::min(dir_bytes(y), cap); };
    if (int rc = plan_passes((long long)above.size(), bytes_of, cap, 1, trace_pass, no_range, kNtTraceBatch)) return rc;
    c->nt_sec[4] = mirp::now() - t;

    // ---- selection: per pair by (score descending, a_start, b_start, bin), greedily; one that overlaps an accepted one of its pair in A and in B goes
    t = mirp::now();
    std::sort(kept.begin(), kept.end(), [](const Kept& x, const Kept& y) {
        const MirpNatsRec &p = x.rec, &q = y.rec;
        if (p.a != q.a) return p.a < q.a;
        if (p.b != q.b) return p.b < q.b;
        if (p.score != q.score) return p.score > q.score;
        if (p.a_start != q.a_start) return p.a_start < q.a_start;
        if (p.b_start != q.b_start) return p.b_start < q.b_start;
        return p.bin < q.bin;
    });
    std::vector<Kept> chosen;
    size_t pair_first = 0;
    long long pairs = 0;
    for (const Kept& kp : kept) {
        if (chosen.size() > pair_first && (chosen[pair_first].rec.a != kp.rec.a || chosen[pair_first].rec.b != kp.rec.b)) pair_first = chosen.size();
        bool hit = false;
        for (size_t z = pair_first; z < chosen.size() && !hit; z++) {
            const MirpNatsRec& ac = chosen[z].rec;
            hit = kp.rec.a_start <= ac.a_end && ac.a_start <= kp.rec.a_end && kp.rec.b_start <= ac.b_end && ac.b_start <= kp.rec.b_end;
        }
        if (hit) continue;
        if (chosen.size() == pair_first) pairs++;
        chosen.push_back(kp);
    }
    std::sort(chosen.begin(), chosen.end(), [](const Kept& x, const Kept& y) {
        const MirpNatsRec &p = x.rec, &q = y.rec;
        if (p.a != q.a) return p.a < q.a;
        if (p.b != q.b) return p.b < q.b;
        if (p.a_start != q.a_start) return p.a_start < q.a_start;
        return p.b_start < q.b_start;
    });
    c->nt_stats[10] = (long long)chosen.size();
    c->nt_stats[11] = pairs;
    for (const Kept& kp : chosen) {
        recs.push_back(kp.rec);
        ops.insert(ops.end(), all_ops.begin() + kp.ops_at, all_ops.begin() + kp.ops_at + kp.n_ops);
        ops_off.push_back((long long)ops.size());
    }
    c->nt_sec[5] = mirp::now() - t;
    return 0;
}

// Device side of the gapped local alignment of queries (predicted precursors) with known sequences (miRBase hairpins): mirp_hairpin_align,
// mirp_hairpin.cpp, with the semantics of DESIGN.md §25.  Integer arithmetic only; every result is a function of the pair and the options.
//
// Codes: A C G U = 0..3, an unknown letter 4 in a query and 5 in a known sequence, the padding 6 (query rows) and 7 (known columns): a padding cell
// only ever holds values strictly below a real cell it derives from (every step into it costs at least 1), so it never holds the maximum.
//
//   score  hp_score_kernel: one lane per known sequence, one wave per block.  The known sequences are sorted by length and stored per wave as
//          word x lane (8 letters of 4 bits to a word), padded to the wave's longest.  The query is wave-uniform and arrives through scalar loads.
//          A lane holds a strip of HP_R query rows (H and E of the column to the left) in registers and streams over its columns; H and F of the
//          strip's last row go to the next strip through a lane-interleaved buffer (one 32-bit word read and one written per column and strip,
//          two buffers that alternate so that the loads do not wait for the stores).  The best cell of a strip is one key under an unsigned maximum,
//          score << 17 | (HP_R - 1 - row) << 12 | 4095 - column: the largest score, then the smallest row, then the smallest column; strips are
//          joined by `>` in ascending order.  A block folds `chunk` queries one after the other, so the boundary buffer is sized by the grid.
//          res[query - q0][known] = score << 32 | end row << 16 | end column; cnt[query] += pairs with score >= min_score.
//   keys   hp_filter_kernel: the hits of the pass as keys, query - q0 << 40 | 32767 - score << 25 | known, sorted by mirp_device_sort_u64 = the
//          output order; hp_cut_kernel keeps the first max_lines of every query (as annotate's cut); hp_hit_kernel turns the kept keys into
//          hit records that hold the pair, the score and the end cell.
//   trace  hp_trace_kernel: one wave per kept hit redoes the DP on q[1 .. q_end] x k[1 .. k_end] row by row, 64 columns at a time.  F and the
//          diagonal need the row above only; E(i, j) = max over j' < j of H~(i, j') - o - (j - j') e with H~ = max(0, diagonal, F) is a prefix
//          maximum over the lanes (a gap opened from a cell that E itself won never beats extending that gap, so H~ may stand for H).  Each cell's
//          byte holds H's source (0 stop, 1 diagonal, 2 E, 3 F), E opened (4) and F opened (8), exactly the comparisons of the definition's
//          traceback; then lane 0 walks back from the end cell and writes the ops backwards from the end of the hit's region, so they stand in
//          forward order, and completes the record.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"

namespace mirp {

#define HP_R MIRP_HAIRPIN_STRIP
#define HP_NEG (-100000)
#define HP_MAXLEN 3000
#define HP_GROUP (1 << 16)      // queries per scoring pass (the key holds 16 bits of query index)

static_assert(HP_R == 16, "the strip's key holds 4 bits of row and its letters come as one 16-byte scalar load");

struct HpScore { int a, b, oe, e; };                     // match, mismatch, gap_open + gap_extend, gap_extend
struct HpWave { long long kw_off; int n_words, pad; };   // first word of the wave's letters (its boundary rows start at 8 x that), words per lane
struct HpJob { long long dir_off, ops_end; };            // first byte of the hit's direction matrix, end of its ops region

// one strip of HP_R rows over all columns of the lane; -> the strip's key
__device__ __forceinline__ unsigned hp_strip(const unsigned* __restrict__ kw, int n_words, const unsigned* __restrict__ rd, unsigned* __restrict__ wr,
                                             const uint4 qw, const bool first, const bool last, const HpScore S) {
    unsigned ql[HP_R];
    const unsigned qv[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int r = 0; r < HP_R; r++) ql[r] = (qv[r >> 2] >> (8 * (r & 3))) & 0xffu;
    int H[HP_R], E[HP_R];
#pragma unroll
    for (int r = 0; r < HP_R; r++) { H[r] = 0; E[r] = HP_NEG; }
    int diag0 = 0;
    unsigned key = 0;
    for (int w = 0; w < n_words; w++) {
        const unsigned word = kw[(long long)w * 64];
#pragma unroll
        for (int cc = 0; cc < 8; cc++) {
            const int j = w * 8 + cc;
            const unsigned kl = (word >> (4 * cc)) & 15u;
            int hup = 0, fup = HP_NEG;
            if (!first) {
                const unsigned v = rd[(long long)j * 64];
                hup = (int)(v & 0xffffu);
                fup = (int)v >> 16;
            }
            int d = diag0;
            diag0 = hup;
            const unsigned cj = 4095u - (unsigned)(j + 1);
#pragma unroll
            for (int r = 0; r < HP_R; r++) {
                const int e = max(H[r] - S.oe, E[r] - S.e);
                const int f = max(hup - S.oe, fup - S.e);
                const int s = kl == ql[r] ? S.a : -S.b;
                const int h = max(max(d + s, e), max(f, 0));
                d = H[r];
                H[r] = h;
                E[r] = e;
                hup = h;
                fup = f;
                key = max(key, ((unsigned)h << 17) + (((unsigned)(HP_R - 1 - r) << 12) + cj));
            }
            if (!last) wr[(long long)j * 64] = (unsigned)hup | ((unsigned)fup << 16);
        }
    }
    return key;
}

// blockIdx.x: the wave of known sequences; blockIdx.y: queries q0 + blockIdx.y * chunk .. of [q0, q1).  carry_a / carry_b: carry_stride words per
// blockIdx.y each.
__global__ __launch_bounds__(64) void hp_score_kernel(
    const unsigned* __restrict__ kwords, const HpWave* __restrict__ waves, const int* __restrict__ korig, const unsigned char* __restrict__ qcodes,
    const long long* __restrict__ q_at, const int* __restrict__ q_len, long long q0, long long q1, long long chunk, HpScore S, int min_score,
    unsigned* __restrict__ carry_a, unsigned* __restrict__ carry_b, long long carry_stride, long long nk, unsigned long long* __restrict__ res,
    unsigned* __restrict__ cnt) {
    const int lane = threadIdx.x;
    const HpWave W = waves[blockIdx.x];
    const unsigned* kw = kwords + W.kw_off + lane;
    const long long cbase = (long long)blockIdx.y * carry_stride + 8 * W.kw_off + lane;
    unsigned* ca = carry_a + cbase;
    unsigned* cb = carry_b + cbase;
    const int ko = korig[(long long)blockIdx.x * 64 + lane];
    const long long qa = q0 + (long long)blockIdx.y * chunk, qb = qa + chunk < q1 ? qa + chunk : q1;
    for (long long q = qa; q < qb; q++) {
        const int n_strips = (q_len[q] + HP_R - 1) / HP_R;
        const uint4* qs = (const uint4*)(qcodes + q_at[q]);
        unsigned best = 0, bi = 0, bj = 0;
        for (int st = 0; st < n_strips; st++) {
            const unsigned key = hp_strip(kw, W.n_words, st & 1 ? cb : ca, st & 1 ? ca : cb, qs[st], st == 0, st == n_strips - 1, S);
            const unsigned sc = key >> 17;
            if (sc > best) {
                best = sc;
                bi = (unsigned)(st * HP_R) + (HP_R - 1 - ((key >> 12) & 15u)) + 1u;
                bj = 4095u - (key & 4095u);
            }
        }
        const bool hit = ko >= 0 && best >= (unsigned)min_score;
        if (ko >= 0) res[(q - q0) * nk + ko] = ((unsigned long long)best << 32) | ((unsigned long long)bi << 16) | bj;
        const unsigned long long b = __ballot(hit);
        if (b && lane == 0) atomicAdd(&cnt[q], (unsigned)__popcll(b));
    }
}

__global__ void hp_filter_kernel(const unsigned long long* __restrict__ res, long long n_pairs, long long nk, int min_score,
                                 unsigned long long* __restrict__ keys, unsigned long long cap, unsigned long long* __restrict__ counter) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n_pairs; i += (long long)gridDim.x * blockDim.x) {
        const unsigned sc = (unsigned)(res[i] >> 32);
        if (sc >= (unsigned)min_score) {
            const unsigned long long at = atomicAdd(counter, 1ull);
            const unsigned long long q = (unsigned long long)(i / nk), k = (unsigned long long)(i % nk);
            if (at < cap) keys[at] = (q << 40) | ((unsigned long long)(32767u - sc) << 25) | k;
        }
    }
}

// sorted keys[0 .. n): key i of query qloc has rank i - run[qloc] in its run and is kept when that is below out[qloc + 1] - out[qloc]
__global__ void hp_cut_kernel(const unsigned long long* __restrict__ keys, long long n, const long long* __restrict__ run, const long long* __restrict__ out,
                              unsigned long long* __restrict__ kept) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const long long q = (long long)(key >> 40), r = i - run[q];
        if (r < out[q + 1] - out[q]) kept[out[q] + r] = key;
    }
}

__global__ void hp_hit_kernel(const unsigned long long* __restrict__ keys, long long n, const unsigned long long* __restrict__ res, long long nk, long long q0,
                              MirpHairpinHit* __restrict__ hits) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const long long q = (long long)(key >> 40), k = (long long)(key & 0x1ffffffull);
        const unsigned long long v = res[q * nk + k];
        MirpHairpinHit h;
        h.query = (int)(q0 + q); h.known = (int)k; h.score = (int)(v >> 32);
        h.q_start = 0; h.q_end = (int)((v >> 16) & 0xffffu); h.k_start = 0; h.k_end = (int)(v & 0xffffu);
        h.matches = h.mismatches = h.gap_opens = h.gap_bases = h.reserved = 0;
        hits[i] = h;
    }
}

// one wave per hit; lane l owns the columns l, l + 64, ... of the row buffers, so they need no barrier
__global__ __launch_bounds__(64) void hp_trace_kernel(const unsigned char* __restrict__ qcodes, const long long* __restrict__ q_at,
                                                      const unsigned char* __restrict__ kcodes, const long long* __restrict__ k_at,
                                                      MirpHairpinHit* __restrict__ hits, const HpJob* __restrict__ jobs, HpScore S,
                                                      unsigned char* __restrict__ dir, char* __restrict__ ops) {
    __shared__ int Hs[HP_MAXLEN + 72], Fs[HP_MAXLEN + 72];
    const int lane = threadIdx.x;
    MirpHairpinHit hit = hits[blockIdx.x];
    const HpJob job = jobs[blockIdx.x];
    const unsigned char* qs = qcodes + q_at[hit.query];
    const unsigned char* ks = kcodes + k_at[hit.known];
    const int n = hit.q_end, m = hit.k_end;
    unsigned char* D = dir + job.dir_off;
    const int n_chunks = (m + 63) / 64;
    for (int c = 0; c < n_chunks; c++) { Hs[c * 64 + lane] = 0; Fs[c * 64 + lane] = HP_NEG; }
    for (int i = 0; i < n; i++) {
        const unsigned ql = qs[i];
        int carry_diag = 0, carry_h = 0, carry_p = 0;          // H(i-1, 0), H(i, 0), H(i, 0) + 0 e
        for (int c = 0; c < n_chunks; c++) {
            const int j0 = c * 64 + lane;                      // the column, 0-based
            const int hup = Hs[j0], fup = Fs[j0];
            int dg = __shfl_up(hup, 1);
            if (lane == 0) dg = carry_diag;
            carry_diag = __shfl(hup, 63);
            const unsigned kl = j0 < m ? ks[j0] : 7u;
            const int f = max(hup - S.oe, fup - S.e);
            const int d = dg + (kl == ql ? S.a : -S.b);
            const int ht = max(max(d, f), 0);
            int p = ht + (j0 + 1) * S.e;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(p, off);
                if (lane >= off) p = max(p, t);
            }
            p = max(p, carry_p);
            int pe = __shfl_up(p, 1);
            if (lane == 0) pe = carry_p;
            carry_p = __shfl(p, 63);
            const int e = pe - S.oe - j0 * S.e;
            const int h = max(ht, e);
            int hl = __shfl_up(h, 1);
            if (lane == 0) hl = carry_h;
            carry_h = __shfl(h, 63);
            const unsigned src = h == 0 ? 0u : h == d ? 1u : h == e ? 2u : 3u;
            const unsigned bits = src | (e == hl - S.oe ? 4u : 0u) | (f == hup - S.oe ? 8u : 0u);
            if (j0 < m) D[(long long)i * m + j0] = (unsigned char)bits;
            Hs[j0] = h;
            Fs[j0] = f;
        }
    }
    __syncthreads();          // (a one-wave block: this is what makes the direction bytes the other lanes wrote visible to lane 0 before the walk)
    if (lane != 0) return;
    int i = n, j = m, state = 0, n_eq = 0, n_x = 0, n_open = 0, n_gap = 0;
    long long w = job.ops_end;
    char prev = 0;
    while (i > 0 && j > 0) {
        const unsigned b = D[(long long)(i - 1) * m + (j - 1)];
        char op;
        if (state == 0) {
            const unsigned src = b & 3u;
            if (src == 0) break;
            if (src != 1) { state = src == 2 ? 1 : 2; continue; }
            op = qs[i - 1] == ks[j - 1] ? '=' : 'X';
            if (op == '=') n_eq++; else n_x++;
            i--; j--;
        } else if (state == 1) {
            op = 'D';
            if (b & 4u) state = 0;
            j--;
        } else {
            op = 'I';
            if (b & 8u) state = 0;
            i--;
        }
        if (op == 'D' || op == 'I') { n_gap++; if (op != prev) n_open++; }
        prev = op;
        ops[--w] = op;
    }
    hit.q_start = i + 1; hit.k_start = j + 1;
    hit.matches = n_eq; hit.mismatches = n_x; hit.gap_opens = n_open; hit.gap_bases = n_gap;
    hits[blockIdx.x] = hit;
}

}  // namespace mirp

namespace {

const long long kHpDefaultCapacity = 1ll << 31;
const long long kHpCarryWords = 1ll << 27;       // the two boundary buffers together hold at most 2 x 4 x this many bytes (unless one slice needs more)

unsigned hp_grid(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 16384)); }

}  // namespace

int mirp_device_hairpin(mirp_ctx* c, const HpSeqs& Q, const HpSeqs& K, const MirpHairpinOpts& o, std::vector<MirpHairpinHit>& hits, std::vector<char>& ops,
                        std::vector<long long>& ops_off) {
    using namespace mirp;
    hipStream_t st = c->stream;
    const long long nq = (long long)Q.len.size(), nk = (long long)K.len.size();
    hits.clear();
    ops.clear();
    ops_off.assign(1, 0);
    c->hp_per_query.assign((size_t)nq, 0);
    for (int i = 0; i < 8; i++) c->hp_stats[i] = 0;
    for (int i = 0; i < 5; i++) c->hp_sec[i] = 0;
    long long sum_q = 0, sum_k = 0;
    for (int L : Q.len) sum_q += L;
    for (int L : K.len) sum_k += L;
    c->hp_stats[0] = nq; c->hp_stats[1] = nk; c->hp_stats[2] = nq * nk; c->hp_stats[3] = sum_q * sum_k;
    if (nq == 0 || nk == 0) return 0;
    const long long cap = c->hp_cap > 0 ? c->hp_cap : kHpDefaultCapacity;
    const HpScore S{o.match, o.mismatch, o.gap_open + o.gap_extend, o.gap_extend};
    const long long K_lines = o.max_lines;

    // the known sequences by (length, index), 64 to a wave, every wave padded to its longest
    double t = mirp::now();
    std::vector<int> perm((size_t)nk);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return K.len[(size_t)a] < K.len[(size_t)b]; });
    const long long n_waves = (nk + 63) / 64;
    std::vector<HpWave> waves((size_t)n_waves);
    std::vector<int> korig((size_t)n_waves * 64, -1);
    long long n_words = 0;
    for (long long w = 0; w < n_waves; w++) {
        const long long last = std::min(nk, (w + 1) * 64) - 1;
        const int words = (K.len[(size_t)perm[(size_t)last]] + 7) / 8;
        waves[(size_t)w] = HpWave{n_words, words, 0};
        n_words += (long long)words * 64;
    }
    std::vector<unsigned> kwords((size_t)n_words, 0x77777777u);
    for (long long s = 0; s < nk; s++) {
        const int k = perm[(size_t)s];
        korig[(size_t)s] = k;
        const unsigned char* cd = K.codes.data() + K.at[(size_t)k];
        unsigned* dst = kwords.data() + waves[(size_t)(s / 64)].kw_off + (s % 64);
        for (int p = 0; p < K.len[(size_t)k]; p++) {
            unsigned& word = dst[(size_t)(p / 8) * 64];
            word = (word & ~(15u << (4 * (p % 8)))) | ((unsigned)cd[p] << (4 * (p % 8)));
        }
    }
    const long long carry_stride = 8 * n_words;
    if (c->hp_q.ensure(Q.codes.size() + 16) || c->hp_qat.ensure(8 * (size_t)nq) || c->hp_qlen.ensure(4 * (size_t)nq) || c->hp_k.ensure(K.codes.size() + 16) ||
        c->hp_kat.ensure(8 * (size_t)nk) || c->hp_kw.ensure(4 * (size_t)n_words) || c->hp_waves.ensure(sizeof(HpWave) * (size_t)n_waves) ||
        c->hp_korig.ensure(4 * (size_t)n_waves * 64) || c->hp_cnt.ensure(4 * (size_t)nq) || c->hp_small.ensure(64))
        return fail(c, -6, "mirp_hairpin_align: device allocation failed (sequences)");
    HIPCHK(c, hipMemcpyAsync(c->hp_q.p, Q.codes.data(), Q.codes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_qat.p, Q.at.data(), 8 * (size_t)nq, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_qlen.p, Q.len.data(), 4 * (size_t)nq, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_k.p, K.codes.data(), K.codes.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_kat.p, K.at.data(), 8 * (size_t)nk, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_kw.p, kwords.data(), 4 * (size_t)n_words, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_waves.p, waves.data(), sizeof(HpWave) * (size_t)n_waves, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->hp_korig.p, korig.data(), 4 * (size_t)n_waves * 64, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->hp_cnt.p, 0, 4 * (size_t)nq, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->hp_sec[0] = mirp::now() - t;

    // ---- scoring passes over ranges of queries whose result rows (8 nk bytes each) fit the capacity
    std::vector<unsigned> cnt;
    std::vector<long long> run, out;
    auto score_pass = [&](long long qa, long long qlast, long long) -> int {
        const long long m = qlast - qa + 1;
        double t0 = mirp::now();
        // blocks: enough to fill the device several times over, as far as the boundary buffers allow
        long long gy = std::max<long long>(1, std::min<long long>({m, (long long)c->n_cu * 128 / n_waves + 1, std::max<long long>(1, kHpCarryWords / carry_stride), 65535ll}));
        const long long chunk = (m + gy - 1) / gy;
        gy = (m + chunk - 1) / chunk;
        if (c->hp_res.ensure(8 * (size_t)(m * nk)) || c->hp_carry.ensure(8 * (size_t)(gy * carry_stride)))
            return fail(c, -6, "mirp_hairpin_align: device allocation failed (a scoring pass)");
        unsigned* carry = (unsigned*)c->hp_carry.p;
        c->note_jobs_per_slot(2, chunk, 1);          // a blockIdx.y serves `chunk` queries in turn
        hipLaunchKernelGGL(hp_score_kernel, dim3((unsigned)n_waves, (unsigned)gy), dim3(64), 0, st, (const unsigned*)c->hp_kw.p, (const HpWave*)c->hp_waves.p,
                           (const int*)c->hp_korig.p, (const unsigned char*)c->hp_q.p, (const long long*)c->hp_qat.p, (const int*)c->hp_qlen.p, qa, qa + m, chunk, S,
                           o.min_score, carry, carry + gy * carry_stride, carry_stride, nk, (unsigned long long*)c->hp_res.p, (unsigned*)c->hp_cnt.p);
        cnt.resize((size_t)m);
        HIPCHK(c, hipMemcpyAsync(cnt.data(), (const unsigned*)c->hp_cnt.p + qa, 4 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        c->hp_sec[1] += mirp::now() - t0;
        c->hp_stats[6]++;
        t0 = mirp::now();
        run.assign((size_t)m + 1, 0);
        out.assign((size_t)m + 1, 0);
        for (long long q = 0; q < m; q++) {
            const long long n = cnt[(size_t)q];
            c->hp_per_query[(size_t)(qa + q)] = n;
            run[(size_t)q + 1] = run[(size_t)q] + n;
            out[(size_t)q + 1] = out[(size_t)q] + (K_lines > 0 ? std::min(n, K_lines) : n);
        }
        const long long total = run[(size_t)m], keep = out[(size_t)m];
        c->hp_stats[4] += total;
        if (total == 0) return 0;
        if (c->hp_keys.ensure(8 * (size_t)total) || c->hp_ktmp.ensure(8 * (size_t)total) || c->hp_hits.ensure(sizeof(MirpHairpinHit) * (size_t)keep))
            return fail(c, -6, "mirp_hairpin_align: device allocation failed (keys)");
        unsigned long long* d_keys = (unsigned long long*)c->hp_keys.p;
        HIPCHK(c, hipMemsetAsync(c->hp_small.p, 0, 8, st));
        hipLaunchKernelGGL(hp_filter_kernel, dim3(hp_grid(m * nk)), dim3(256), 0, st, (const unsigned long long*)c->hp_res.p, m * nk, nk, o.min_score, d_keys,
                           (unsigned long long)total, (unsigned long long*)c->hp_small.p);
        unsigned long long found = 0;
        HIPCHK(c, hipMemcpyAsync(&found, c->hp_small.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if ((long long)found != total) return fail(c, -5, "mirp_hairpin_align: the filter found a different number of hits than the scoring kernel counted");
        int qbits = 0;
        while ((1ll << qbits) < m) qbits++;
        if (int rc = mirp_device_sort_u64(c, d_keys, (unsigned long long*)c->hp_ktmp.p, total, 0, (40 + qbits + 7) / 8 * 8)) return rc;
        const unsigned long long* src = d_keys;
        if (keep != total) {
            if (c->hp_run.ensure(8 * ((size_t)m + 1)) || c->hp_out.ensure(8 * ((size_t)m + 1)) || c->hp_kept.ensure(8 * (size_t)keep))
                return fail(c, -6, "mirp_hairpin_align: device allocation failed (cut)");
            HIPCHK(c, hipMemcpyAsync(c->hp_run.p, run.data(), 8 * ((size_t)m + 1), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(c->hp_out.p, out.data(), 8 * ((size_t)m + 1), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(hp_cut_kernel, dim3(hp_grid(total)), dim3(256), 0, st, (const unsigned long long*)d_keys, total, (const long long*)c->hp_run.p,
                               (const long long*)c->hp_out.p, (unsigned long long*)c->hp_kept.p);
            src = (const unsigned long long*)c->hp_kept.p;
        }
        hipLaunchKernelGGL(hp_hit_kernel, dim3(hp_grid(keep)), dim3(256), 0, st, src, keep, (const unsigned long long*)c->hp_res.p, nk, qa, (MirpHairpinHit*)c->hp_hits.p);
        const size_t at = hits.size();
        hits.resize(at + (size_t)keep);
        HIPCHK(c, hipMemcpyAsync(hits.data() + at, c->hp_hits.p, sizeof(MirpHairpinHit) * (size_t)keep, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        c->hp_sec[2] += mirp::now() - t0;
        return 0;
    };
    auto no_range = [&](long long, unsigned long long, unsigned long long, long long*) -> int { return fail(c, -5, "mirp_hairpin_align: pass plan"); };
    // a query whose row alone exceeds the capacity counts as one that just fits: it gets a pass of its own
    if (int rc = plan_passes(nq, [&](long long) { return std::min(8 * nk, cap); }, cap, 1, score_pass, no_range, HP_GROUP)) return rc;

    // ---- traceback passes over ranges of hits whose direction matrices (q_end x k_end bytes each) fit the capacity
    const long long n_hits = (long long)hits.size();
    ops_off.assign((size_t)n_hits + 1, 0);
    std::vector<HpJob> jobs;
    std::vector<char> region;
    auto dir_bytes = [&](long long h) { return (long long)hits[(size_t)h].q_end * hits[(size_t)h].k_end; };
    auto trace_pass = [&](long long ha, long long hlast, long long) -> int {
        const long long m = hlast - ha + 1;
        double t0 = mirp::now();
        jobs.resize((size_t)m);
        long long dir_at = 0, ops_at = 0;
        for (long long h = 0; h < m; h++) {
            ops_at += hits[(size_t)(ha + h)].q_end + hits[(size_t)(ha + h)].k_end;
            jobs[(size_t)h] = HpJob{dir_at, ops_at};
            dir_at += dir_bytes(ha + h);
        }
        if (c->hp_hits.ensure(sizeof(MirpHairpinHit) * (size_t)m) || c->hp_jobs.ensure(sizeof(HpJob) * (size_t)m) || c->hp_dir.ensure((size_t)dir_at + 16) ||
            c->hp_ops.ensure((size_t)ops_at + 16))
            return fail(c, -6, "mirp_hairpin_align: device allocation failed (a traceback pass)");
        HIPCHK(c, hipMemcpyAsync(c->hp_hits.p, hits.data() + ha, sizeof(MirpHairpinHit) * (size_t)m, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->hp_jobs.p, jobs.data(), sizeof(HpJob) * (size_t)m, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(hp_trace_kernel, dim3((unsigned)m), dim3(64), 0, st, (const unsigned char*)c->hp_q.p, (const long long*)c->hp_qat.p,
                           (const unsigned char*)c->hp_k.p, (const long long*)c->hp_kat.p, (MirpHairpinHit*)c->hp_hits.p, (const HpJob*)c->hp_jobs.p, S,
                           (unsigned char*)c->hp_dir.p, (char*)c->hp_ops.p);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        c->hp_sec[3] += mirp::now() - t0;
        t0 = mirp::now();
        region.resize((size_t)ops_at);
        HIPCHK(c, hipMemcpyAsync(hits.data() + ha, c->hp_hits.p, sizeof(MirpHairpinHit) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(region.data(), c->hp_ops.p, (size_t)ops_at, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (long long h = 0; h < m; h++) {
            const MirpHairpinHit& r = hits[(size_t)(ha + h)];
            const long long n = (long long)r.matches + r.mismatches + r.gap_bases, end = jobs[(size_t)h].ops_end;
            if (n < 1 || n > (long long)r.q_end + r.k_end) return fail(c, -5, "mirp_hairpin_align: a traceback of impossible length");
            ops.insert(ops.end(), region.begin() + (end - n), region.begin() + end);
            ops_off[(size_t)(ha + h) + 1] = (long long)ops.size();
        }
        c->hp_sec[4] += mirp::now() - t0;
        c->hp_stats[7]++;
        return 0;
    };
    // at most 2^20 hits to a pass (the grid); a hit whose matrix alone exceeds the capacity gets a pass of its own
    if (int rc = plan_passes(n_hits, [&](long long h) { return std::min(std::max(dir_bytes(h), 1ll), cap); }, cap, 1, trace_pass, no_range, 1 << 20)) return rc;
    c->hp_stats[5] = c->hp_stats[6] + c->hp_stats[7];
    return 0;
}

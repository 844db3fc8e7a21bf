// Fold dedup: the windows of one mirp_fold whose bytes repeat an earlier window's are found on the device, skipped by the
// fold (their length is handed to it as 0, which every fill kernel takes as an empty window) and given their representative's results afterwards.
//
//   fold_dup_hash_kernel     a wave per window: 64-bit hash of (length, bytes), then the lowest window index per hash in an open-addressing table
//   fold_dup_resolve_kernel  a wave per window: the lowest index with its hash is a candidate only; length and every byte are compared before it is
//                            taken.  A collision can cost a missed duplicate, never a wrong merge.
//   fold_dup_copy_kernel     a wave per duplicate: summary, structure lines and structure text of the representative into the duplicate's slots
//   fold_dup_count_kernel    one workgroup: the duplicates of the windows on a (short) hand-off list, for mirp_last_fold_fallbacks / _dense
//
// The map is a pure function of the input.  The table holds one slot per distinct hash, whichever thread claims it first, and keeps the maximum of
// 0x7fffffff - index over the windows with that hash: integer maxima do not depend on the order they arrive in, and a probe sequence finds the slot
// of a hash wherever the races put it, because slots are never released.
#include <hip/hip_runtime.h>
#include "mirp_internal.h"

namespace mirp {

namespace {

constexpr unsigned long long DUP_KEY_BIT = 1ull << 63;      // set in every stored hash: 0 is the empty slot

__device__ __forceinline__ unsigned long long dup_mix(unsigned long long x) {      // the splitmix64 finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void fold_dup_hash_kernel(const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ lens,
                                                            int n_win, int hash_bits, unsigned table_mask, unsigned long long* __restrict__ hash,
                                                            unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_win) return;      // wave-uniform
    const unsigned char* s = seqs + offs[w];
    const int n = lens[w];
    // every position contributes mix(position, byte); the contributions are xor'ed, so the lanes' shares combine in any order
    unsigned long long acc = 0;
    for (int x = lane; x < n; x += 64) acc ^= dup_mix((((unsigned long long)x << 8) | s[x]) + 0x9e3779b97f4a7c15ull);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc ^= __shfl_xor(acc, o);
    unsigned long long h = dup_mix(acc ^ ((unsigned long long)(unsigned)n * 0xd6e8feb86659fd93ull));
    if (hash_bits > 0 && hash_bits < 63) h &= (1ull << hash_bits) - 1ull;      // tests: collisions everywhere
    h |= DUP_KEY_BIT;
    if (lane != 0) return;
    hash[w] = h;
    // at most one slot per distinct hash and at most n_win hashes in a table of >= 2 n_win slots: the probe ends
    for (unsigned slot = (unsigned)h & table_mask, tries = 0; tries <= table_mask; slot = (slot + 1) & table_mask, tries++) {
        const unsigned long long prev = atomicCAS(&keys[slot], 0ull, h);
        if (prev == 0ull || prev == h) { atomicMax(&vals[slot], 0x7fffffffu - (unsigned)w); break; }
    }
}

__global__ __launch_bounds__(256) void fold_dup_resolve_kernel(const unsigned char* __restrict__ seqs, const long long* __restrict__ offs, const int* __restrict__ lens,
                                                               int n_win, unsigned table_mask, const unsigned long long* __restrict__ hash,
                                                               const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                               int* __restrict__ dup_of, int* __restrict__ fold_lens, int* __restrict__ n_dup,
                                                               unsigned* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_win) return;      // wave-uniform
    const int n = lens[w];
    const unsigned long long h = hash[w];
    int cand = -1;      // the same walk in every lane
    for (unsigned slot = (unsigned)h & table_mask, tries = 0; tries <= table_mask; slot = (slot + 1) & table_mask, tries++) {
        const unsigned long long k = keys[slot];
        if (k == h) { cand = (int)(0x7fffffffu - vals[slot]); break; }
        if (k == 0ull) break;
    }
    bool same = cand >= 0 && cand < w && n >= 1 && lens[cand] == n;      // wave-uniform
    if (same) {
        const unsigned char* a = seqs + offs[w];
        const unsigned char* b = seqs + offs[cand];
        bool diff = false;
        for (int x = lane; x < n; x += 64) diff |= a[x] != b[x];
        same = __ballot(diff) == 0ull;
    }
    if (lane == 0) {
        dup_of[w] = same ? cand : -1;
        fold_lens[w] = same ? 0 : n;
        if (same) { atomicAdd(&n_dup[cand], 1); atomicAdd(total, 1u); }
    }
}

__global__ __launch_bounds__(256) void fold_dup_copy_kernel(const int* __restrict__ dup_of, int n_win, int max_lines, int ss_stride, MirpFoldLine* __restrict__ lines,
                                                            char* __restrict__ ss, int* __restrict__ nlines, int* __restrict__ mfe, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_win) return;      // wave-uniform
    const int r = dup_of[w];
    if (r < 0) return;
    const int nl = nlines[r];
    if (lane == 0) { nlines[w] = nl; mfe[w] = mfe[r]; status[w] = status[r]; }
    const int rows = nl < 0 ? 0 : nl < max_lines ? nl : max_lines;      // a window over the line capacity reports the lines it needs and holds the first max_lines
    // MirpFoldLine is 16 bytes and holds no absolute offset; ss_stride is a multiple of 8 and the buffers come from hipMalloc
    const int4* ls = reinterpret_cast<const int4*>(lines + (size_t)r * max_lines);
    int4* ld = reinterpret_cast<int4*>(lines + (size_t)w * max_lines);
    for (int x = lane; x < rows; x += 64) ld[x] = ls[x];
    const unsigned long long* ts = reinterpret_cast<const unsigned long long*>(ss + (size_t)r * max_lines * ss_stride);
    unsigned long long* td = reinterpret_cast<unsigned long long*>(ss + (size_t)w * max_lines * ss_stride);
    const int words = rows * (ss_stride >> 3);
    for (int x = lane; x < words; x += 64) td[x] = ts[x];
}

__global__ __launch_bounds__(256) void fold_dup_count_kernel(const int* __restrict__ list, const unsigned* __restrict__ list_len, int base, const int* __restrict__ n_dup,
                                                             unsigned* __restrict__ out, int accumulate, const unsigned* __restrict__ total_src,
                                                             unsigned* __restrict__ total_dst) {
    __shared__ unsigned sum;
    if (threadIdx.x == 0) sum = 0;
    __syncthreads();
    const unsigned n = *list_len;
    unsigned mine = 0;
    for (unsigned k = threadIdx.x; k < n; k += blockDim.x) mine += (unsigned)n_dup[base + list[k]];
    if (mine) atomicAdd(&sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (accumulate) { if (sum) atomicAdd(out, sum); }
        else *out = sum;
        if (total_dst) *total_dst = *total_src;
    }
}

}  // namespace

FoldDedupLayout fold_dedup_layout(long long n_win) {
    FoldDedupLayout L;
    unsigned long long t = 64;
    while (t < 2ull * (unsigned long long)n_win) t <<= 1;
    const size_t nw = (size_t)n_win;
    L.table = (unsigned)t;
    // cleared before every use: the count, the duplicates per representative, the table
    L.total = 0;
    L.keys = 64;
    L.vals = L.keys + 8 * (size_t)t;
    L.n_dup = L.vals + 4 * (size_t)t;
    L.clear_bytes = L.n_dup + 4 * nw;
    // written in full by the kernels
    L.hash = (L.clear_bytes + 7) & ~(size_t)7;
    L.dup_of = L.hash + 8 * nw;
    L.fold_lens = L.dup_of + 4 * nw;
    L.bytes = L.fold_lens + 4 * nw;
    return L;
}

hipError_t launch_fold_dedup_find(hipStream_t st, const unsigned char* seqs, const long long* offs, const int* lens, int n_win, int hash_bits, char* buf,
                                  const FoldDedupLayout& L) {
    if (hipError_t e = hipMemsetAsync(buf, 0, L.clear_bytes, st)) return e;
    const dim3 grid((unsigned)((n_win + 3) / 4)), block(256);
    hipLaunchKernelGGL(fold_dup_hash_kernel, grid, block, 0, st, seqs, offs, lens, n_win, hash_bits, L.table - 1u, (unsigned long long*)(buf + L.hash),
                       (unsigned long long*)(buf + L.keys), (unsigned*)(buf + L.vals));
    hipLaunchKernelGGL(fold_dup_resolve_kernel, grid, block, 0, st, seqs, offs, lens, n_win, L.table - 1u, (const unsigned long long*)(buf + L.hash),
                       (const unsigned long long*)(buf + L.keys), (const unsigned*)(buf + L.vals), (int*)(buf + L.dup_of), (int*)(buf + L.fold_lens),
                       (int*)(buf + L.n_dup), (unsigned*)(buf + L.total));
    return hipGetLastError();
}

hipError_t launch_fold_dedup_copy(hipStream_t st, const int* dup_of, int n_win, int max_lines, int ss_stride, MirpFoldLine* lines, char* ss, int* nlines, int* mfe,
                                  int* status) {
    hipLaunchKernelGGL(fold_dup_copy_kernel, dim3((unsigned)((n_win + 3) / 4)), dim3(256), 0, st, dup_of, n_win, max_lines, ss_stride, lines, ss, nlines, mfe, status);
    return hipGetLastError();
}

hipError_t launch_fold_dedup_count(hipStream_t st, const int* list, const unsigned* list_len, int base, const int* n_dup, unsigned* out, bool accumulate,
                                   const unsigned* total_src, unsigned* total_dst) {
    hipLaunchKernelGGL(fold_dup_count_kernel, dim3(1), dim3(256), 0, st, list, list_len, base, n_dup, out, accumulate ? 1 : 0, total_src, total_dst);
    return hipGetLastError();
}

}  // namespace mirp

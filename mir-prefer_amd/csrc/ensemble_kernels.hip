// Partition function of whole sequences (McCaskill inside / outside fold): one workgroup folds one sequence, the cells of an
// anti-diagonal d = j - i run in parallel (a thread per cell, one barrier per diagonal), the inside pass from d = 4 outwards, the outside pass
// from d = n - 1 inwards.  Every table holds ln Q (FP64); a sum is a max-shifted sum of exponentials kept as (max, sum) and walked in a fixed
// order by one thread, so a cell's value depends on nothing but the sequence: no atomics, no dependence on the grid or on the other jobs.
// A table is stored by diagonals (row d holds the cells (i, i + d), i = 0 .. n - d - 1, at en_off(n, d) + i), so the threads of a diagonal read
// consecutive doubles in all three O(n) sums (Qmm, its two adjoints).  Staged in LDS: the coded sequence, the small energy tables as integers
// (a Boltzmann factor in the ln domain is the energy times -1 / (100 kT): the integer sum of a loop's terms is exact and is scaled once), and, for
// sequences of at most MIRP_ENSEMBLE_RING_N nt, the 31 diagonals of Qb (inside) / of its adjoint (outside) that the interior loops of a diagonal re-read,
// in a ring of 33 rows (31 read + the one before + the one written).  Longer sequences read them from the slab (L2).
#include <hip/hip_runtime.h>
#include <cstring>
#include "fold_device.h"
#include "mirp_ctx.h"
#include "ensemble_device.h"

namespace {

constexpr double EN_NEG = -1.0e30;      // ln 0: every real ln Q lies within +-1e5, sums of a few EN_NEG stay finite
constexpr double EN_NEGH = -0.5e30;     // below this a term is nothing
constexpr int EN_RING_ROWS = 33;         // a row's stride: the longest ring sequence of the launch, rounded up to 8 (250 nt: 2 workgroups per CU)
constexpr int EN_NT_RING = 320, EN_NT_GEN = 1024, EN_NT_RED = 256;
constexpr int EN_SMAX = 3008;
static_assert(MIRP_ENSEMBLE_RING_N <= 304, "the ring kernels stage 304 codes");

enum { T_QB = 0, T_QM1, T_U, T_QM, T_QMM, T_PB, T_A1, T_AU, T_AMM, EN_TABLES };


// a sum of exponentials as (max, sum of exp(x - max)); terms arrive in a fixed order
struct Lse {
    double m = EN_NEG, s = 0.0;
    __device__ __forceinline__ void add(double x) {
        if (x > EN_NEGH) {
            if (x > m) { s = s * exp(m - x) + 1.0; m = x; }
            else s += exp(x - m);
        }
    }
    __device__ __forceinline__ void merge(double m2, double s2) {
        if (s2 > 0.0) {
            if (m2 > m) { s = s * exp(m - m2) + s2; m = m2; }
            else s += s2 * exp(m2 - m);
        }
    }
    __device__ __forceinline__ double value() const { return s > 0.0 ? m + log(s) : EN_NEG; }
};
__device__ __forceinline__ double lse2(double a, double b) {
    Lse l;
    l.add(a);
    l.add(b);
    return l.value();
}

// the sum over the block of every thread's (max, sum), by a fixed tree over the thread index; every thread gets the value
__device__ inline double block_lse(Lse l, double* rm, double* rs, int tid, int nt) {
    rm[tid] = l.m;
    rs[tid] = l.s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (tid < w && tid + w < nt) {
            Lse a;
            a.m = rm[tid]; a.s = rs[tid];
            a.merge(rm[tid + w], rs[tid + w]);
            rm[tid] = a.m; rs[tid] = a.s;
        }
        __syncthreads();
    }
    Lse r;
    r.m = rm[0]; r.s = rs[0];
    const double v = r.value();
    __syncthreads();
    return v;
}

template <bool RING>
struct EnLds {
    EnTables T;
    double rm[RING ? EN_NT_RING : EN_NT_GEN], rs[RING ? EN_NT_RING : EN_NT_GEN];
    unsigned char S[RING ? 304 : EN_SMAX];
};

// ring row of diagonal d
__device__ __forceinline__ int ring_row(int d) { return d % EN_RING_ROWS; }

template <bool RING>
__global__ void __launch_bounds__(RING ? EN_NT_RING : EN_NT_GEN)
en_inside_kernel(const FoldParams* __restrict__ P, const unsigned char* __restrict__ codes, const EnJob* __restrict__ jobs, double* __restrict__ slab, int ring_stride) {
    extern __shared__ __align__(16) unsigned char en_smem[];
    EnLds<RING>& L = *(EnLds<RING>*)en_smem;
    double* ring = (double*)(en_smem + sizeof(EnLds<RING>));
    const EnJob J = jobs[blockIdx.x];
    const int n = J.n, tid = threadIdx.x, nt = blockDim.x;
    const int tsz = en_off(n, n);
    double* base = slab + J.slab_off;
    double *Qb = base + (size_t)T_QB * tsz, *Qm1 = base + (size_t)T_QM1 * tsz, *U = base + (size_t)T_U * tsz, *Qm = base + (size_t)T_QM * tsz,
           *Qmm = base + (size_t)T_QMM * tsz, *Q5 = base + (size_t)EN_TABLES * tsz;
    en_stage(&L.T, L.S, P, codes + J.code_off, n, tid, nt);
    const unsigned char* S = L.S;
    const EnTables& T = L.T;
    const int low = en_off(n, n < 4 ? n : 4);
    for (int x = tid; x < low; x += nt) { Qb[x] = EN_NEG; Qm1[x] = EN_NEG; U[x] = EN_NEG; Qm[x] = EN_NEG; Qmm[x] = EN_NEG; }
    __syncthreads();
    for (int d = 4; d < n; d++) {
        const int row = en_off(n, d), row1 = en_off(n, d - 1), row2 = en_off(n, d - 2);
        const int rd = RING ? ring_row(d) : 0;
        for (int i = tid; i < n - d; i += nt) {
            const int j = i + d;
            const int type = mirp::pair_type(S[i], S[j]);
            double qb = EN_NEG;
            if (type) {
                Lse l;
                l.add(EN_G * en_hairpin(T, P, S, i, j, type));
                const int n1max = d - 6 < 30 ? d - 6 : 30;          // q - p >= 4 with n2 = 0
                for (int n1 = 0; n1 <= n1max; n1++) {
                    const int p = i + 1 + n1;
                    int n2max = 30 - n1;
                    if (n2max > d - 6 - n1) n2max = d - 6 - n1;
                    for (int n2 = 0; n2 <= n2max; n2++) {
                        const int q = j - 1 - n2;
                        const int t2 = mirp::pair_type(S[p], S[q]);
                        if (!t2) continue;
                        const int u = n1 + n2;
                        double in;
                        if (RING) {
                            int r = rd - 2 - u;
                            if (r < 0) r += EN_RING_ROWS;
                            in = ring[r * ring_stride + p];
                        } else in = Qb[en_off(n, d - 2 - u) + p];
                        if (in <= EN_NEGH) continue;
                        l.add(in + EN_G * en_intloop(T, P, n1, n2, type, mirp::rtype_of(t2), S[i + 1], S[j - 1], S[p - 1], S[q + 1]));
                    }
                }
                l.add(Qmm[row2 + i + 1] + EN_G * (T.ML_closing + en_mlstem(T, mirp::rtype_of(type), S[j - 1], S[i + 1])));
                qb = l.value();
            }
            double q1 = Qm1[row1 + i];
            if (type) q1 = lse2(q1, qb + EN_G * en_mlstem(T, type, i > 0 ? S[i - 1] : -1, j < n - 1 ? S[j + 1] : -1));
            const double u = lse2(U[row1 + i + 1], q1);
            Lse mm;
            for (int k = i + 5; k <= j - 4; k++) mm.add(Qm[en_off(n, k - 1 - i) + i] + Qm1[en_off(n, j - k) + k]);
            const double qmm = mm.value();
            Qb[row + i] = qb;
            if (RING) ring[rd * ring_stride + i] = qb;
            Qm1[row + i] = q1;
            U[row + i] = u;
            Qmm[row + i] = qmm;
            Qm[row + i] = lse2(u, qmm);
        }
        __syncthreads();
    }
    // exterior prefixes: Q5[j] = ln of the partition function of [0, j]
    for (int j = 0; j < n; j++) {
        Lse l;
        for (int k = tid; k <= j - 4; k += nt) {
            const int t = mirp::pair_type(S[k], S[j]);
            if (t) l.add((k > 0 ? Q5[k - 1] : 0.0) + Qb[en_off(n, j - k) + k] + EN_G * en_extloop(T, t, k > 0 ? S[k - 1] : -1, j < n - 1 ? S[j + 1] : -1));
        }
        const double r = block_lse(l, L.rm, L.rs, tid, nt);
        if (tid == 0) Q5[j] = lse2(j > 0 ? Q5[j - 1] : 0.0, r);
        __syncthreads();
    }
}

template <bool RING>
__global__ void __launch_bounds__(RING ? EN_NT_RING : EN_NT_GEN)
en_outside_kernel(const FoldParams* __restrict__ P, const unsigned char* __restrict__ codes, const EnJob* __restrict__ jobs, double* __restrict__ slab, int ring_stride) {
    extern __shared__ __align__(16) unsigned char en_smem[];
    EnLds<RING>& L = *(EnLds<RING>*)en_smem;
    double* ring = (double*)(en_smem + sizeof(EnLds<RING>));
    const EnJob J = jobs[blockIdx.x];
    const int n = J.n, tid = threadIdx.x, nt = blockDim.x;
    const int tsz = en_off(n, n);
    double* base = slab + J.slab_off;
    const double *Qb = base + (size_t)T_QB * tsz, *Qm1 = base + (size_t)T_QM1 * tsz, *Qm = base + (size_t)T_QM * tsz, *Q5 = base + (size_t)EN_TABLES * tsz;
    double *Pb = base + (size_t)T_PB * tsz, *A1 = base + (size_t)T_A1 * tsz, *AU = base + (size_t)T_AU * tsz, *Amm = base + (size_t)T_AMM * tsz,
           *P5 = base + (size_t)EN_TABLES * tsz + n;
    en_stage(&L.T, L.S, P, codes + J.code_off, n, tid, nt);
    const unsigned char* S = L.S;
    const EnTables& T = L.T;
    __syncthreads();
    // exterior suffixes: P5[j] = dZ / dQ5[j] = ln of the partition function of [j + 1, n - 1]
    if (tid == 0) P5[n - 1] = 0.0;
    __syncthreads();
    for (int jp = n - 2; jp >= 0; jp--) {
        const int k = jp + 1;
        Lse l;
        for (int j = k + 4 + tid; j < n; j += nt) {
            const int t = mirp::pair_type(S[k], S[j]);
            if (t) l.add(P5[j] + Qb[en_off(n, j - k) + k] + EN_G * en_extloop(T, t, S[k - 1], j < n - 1 ? S[j + 1] : -1));
        }
        const double r = block_lse(l, L.rm, L.rs, tid, nt);
        if (tid == 0) P5[jp] = lse2(P5[jp + 1], r);
        __syncthreads();
    }
    for (int d = n - 1; d >= 4; d--) {
        const int row = en_off(n, d), rowp1 = en_off(n, d + 1), rowp2 = en_off(n, d + 2);
        const int rd = RING ? ring_row(d) : 0;
        for (int i = tid; i < n - d; i += nt) {
            const int j = i + d;
            // adjoint of Qm(i,j): Qmm(i,j') = sum_k Qm(i,k-1) Qm1(k,j') with k = j + 1
            Lse lm;
            for (int jq = j + 5; jq < n; jq++) lm.add(Amm[en_off(n, jq - i) + i] + Qm1[en_off(n, jq - j - 1) + j + 1]);
            const double am = lm.value();
            // adjoint of Qmm(i,j): Qm = U + Qmm, and the multiloop closed by (i-1, j+1)
            double amm = am;
            if (i >= 1 && j + 1 < n) {
                const int t = mirp::pair_type(S[i - 1], S[j + 1]);
                if (t) amm = lse2(amm, Pb[rowp2 + i - 1] + EN_G * (T.ML_closing + en_mlstem(T, mirp::rtype_of(t), S[j], S[i])));
            }
            // adjoint of U(i,j): U(i-1,j) = U(i,j) + Qm1(i-1,j), Qm = U + Qmm
            const double au = lse2(i >= 1 ? AU[rowp1 + i - 1] : EN_NEG, am);
            // adjoint of Qm1(i,j): Qm1(i,j+1) = Qm1(i,j) + .., U(i,j) = .. + Qm1(i,j), Qmm(i',j) = sum_k Qm(i',k-1) Qm1(k,j) with k = i
            Lse l1;
            l1.add(j + 1 < n ? A1[rowp1 + i] : EN_NEG);
            l1.add(au);
            for (int ip = 0; ip <= i - 5; ip++) l1.add(Amm[en_off(n, j - ip) + ip] + Qm[en_off(n, i - 1 - ip) + ip]);
            const double a1 = l1.value();
            const int type = mirp::pair_type(S[i], S[j]);
            double pb = EN_NEG;
            if (type) {
                Lse l;
                l.add((i > 0 ? Q5[i - 1] : 0.0) + P5[j] + EN_G * en_extloop(T, type, i > 0 ? S[i - 1] : -1, j < n - 1 ? S[j + 1] : -1));
                const int rt = mirp::rtype_of(type);
                const int n1max = i - 1 < 30 ? i - 1 : 30;
                for (int n1 = 0; n1 <= n1max; n1++) {
                    const int p = i - 1 - n1;
                    int n2max = 30 - n1;
                    if (n2max > n - 2 - j) n2max = n - 2 - j;
                    for (int n2 = 0; n2 <= n2max; n2++) {
                        const int q = j + 1 + n2;
                        const int t2 = mirp::pair_type(S[p], S[q]);
                        if (!t2) continue;
                        const int u = n1 + n2;
                        double out;
                        if (RING) {
                            int r = rd + 2 + u;
                            if (r >= EN_RING_ROWS) r -= EN_RING_ROWS;
                            if (r >= EN_RING_ROWS) r -= EN_RING_ROWS;
                            out = ring[r * ring_stride + p];
                        } else out = Pb[en_off(n, d + 2 + u) + p];
                        if (out <= EN_NEGH) continue;
                        l.add(out + EN_G * en_intloop(T, P, n1, n2, t2, rt, S[p + 1], S[q - 1], S[i - 1], S[j + 1]));
                    }
                }
                l.add(a1 + EN_G * en_mlstem(T, type, i > 0 ? S[i - 1] : -1, j < n - 1 ? S[j + 1] : -1));
                pb = l.value();
            }
            Pb[row + i] = pb;
            if (RING) ring[rd * ring_stride + i] = pb;
            A1[row + i] = a1;
            AU[row + i] = au;
            Amm[row + i] = amm;
        }
        __syncthreads();
    }
}

// p(i,j) = exp(ln Qb + ln dZ/dQb - ln Z) replaces the adjoint in the slab; the sums over the cells go to the record, the pairs with p > 0.5 to the text
__global__ void __launch_bounds__(EN_NT_RED)
en_reduce_kernel(const EnJob* __restrict__ jobs, double* __restrict__ slab, const int* __restrict__ d_mfe, MirpEnsembleRec* __restrict__ recs, char* __restrict__ texts) {
    __shared__ double s_div[EN_NT_RED], s_cd[EN_NT_RED];
    __shared__ int s_cnt[EN_NT_RED];
    const EnJob J = jobs[blockIdx.x];
    const int n = J.n, tid = threadIdx.x, nt = blockDim.x;          // (launched with EN_NT_RED threads: the order of the sums is fixed)
    const int tsz = en_off(n, n);
    double* base = slab + J.slab_off;
    const double* Qb = base + (size_t)T_QB * tsz;
    double* Pb = base + (size_t)T_PB * tsz;
    const double lnz = base[(size_t)EN_TABLES * tsz + n - 1];
    char* text = texts + J.text_off;
    for (int x = tid; x <= n; x += nt) text[x] = x < n ? '.' : 0;
    __syncthreads();
    double div = 0.0, cd = 0.0;
    int cnt = 0;
    for (int d = 4; d < n; d++) {
        const int row = en_off(n, d);
        for (int i = tid; i < n - d; i += nt) {
            const double p = exp(Qb[row + i] + Pb[row + i] - lnz);
            Pb[row + i] = p;
            div += p * (1.0 - p);
            if (p > 0.5) { cd += 1.0 - p; cnt++; text[i] = '('; text[i + d] = ')'; }
            else cd += p;
        }
    }
    s_div[tid] = div; s_cd[tid] = cd; s_cnt[tid] = cnt;
    __syncthreads();
    for (int w = EN_NT_RED / 2; w > 0; w >>= 1) {
        if (tid < w && tid + w < nt) { s_div[tid] += s_div[tid + w]; s_cd[tid] += s_cd[tid + w]; s_cnt[tid] += s_cnt[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        MirpEnsembleRec r;
        r.len = n;
        r.mfe = d_mfe[J.rec];
        r.efe = 0.0 - EN_KT * lnz;
        r.mfe_freq = exp((r.efe - r.mfe / 100.0) / EN_KT);
        r.diversity = 2.0 * s_div[0];
        r.centroid_dist = s_cd[0];
        r.centroid_pairs = s_cnt[0];
        r.reserved = 0;
        recs[J.rec] = r;
    }
}

// the pairs with p >= cutoff, a thread per row i (j ascending): counts per row first (d_out null), then the entries at the rows' offsets
__global__ void __launch_bounds__(EN_NT_RED)
en_bpp_kernel(const EnJob* __restrict__ jobs, const double* __restrict__ slab, double cutoff, int* __restrict__ row_cnt, const long long* __restrict__ row_at,
              MirpBpp* __restrict__ d_out) {
    const EnJob J = jobs[blockIdx.x];
    const int n = J.n;
    const double* Pb = slab + J.slab_off + (size_t)T_PB * en_off(n, n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        long long at = d_out ? row_at[J.row_off + i] : 0;
        int cnt = 0;
        for (int d = 4; i + d < n; d++) {
            const double p = Pb[en_off(n, d) + i];
            if (p >= cutoff) {
                if (d_out) d_out[at++] = MirpBpp{J.rec, i + 1, i + d + 1, 0, p};
                cnt++;
            }
        }
        if (!d_out) row_cnt[J.row_off + i] = cnt;
    }
}

}  // namespace

size_t mirp_ensemble_slab_doubles(int n) { return (size_t)EN_TABLES * ((size_t)n * (n + 1) / 2) + 2 * (size_t)n + 2; }

int mirp_device_ensemble_fold(mirp_ctx* c, const unsigned char* d_codes, const EnJob* d_jobs, int n_ring, int n_jobs, int max_ring_n, double* d_slab) {
    // jobs [0, n_ring): at most MIRP_ENSEMBLE_RING_N nt (max_ring_n the longest), the ring in LDS; the rest reads the slab
    if (n_ring > 0) {
        if (max_ring_n < 1 || max_ring_n > MIRP_ENSEMBLE_RING_N) return fail(c, -1, "mirp_device_ensemble_fold: bad argument");
        const int stride = (max_ring_n + 7) / 8 * 8;
        const size_t lds = sizeof(EnLds<true>) + sizeof(double) * EN_RING_ROWS * stride;
        static_assert(sizeof(EnLds<true>) % 8 == 0 && sizeof(EnLds<true>) + sizeof(double) * EN_RING_ROWS * 304 <= 160 * 1024, "LDS budget");
        HIPCHK(c, hipFuncSetAttribute((const void*)en_inside_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPCHK(c, hipFuncSetAttribute((const void*)en_outside_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        en_inside_kernel<true><<<n_ring, EN_NT_RING, lds, c->stream>>>(c->d_params, d_codes, d_jobs, d_slab, stride);
        en_outside_kernel<true><<<n_ring, EN_NT_RING, lds, c->stream>>>(c->d_params, d_codes, d_jobs, d_slab, stride);
    }
    if (n_jobs > n_ring) {
        en_inside_kernel<false><<<n_jobs - n_ring, EN_NT_GEN, sizeof(EnLds<false>), c->stream>>>(c->d_params, d_codes, d_jobs + n_ring, d_slab, 0);
        en_outside_kernel<false><<<n_jobs - n_ring, EN_NT_GEN, sizeof(EnLds<false>), c->stream>>>(c->d_params, d_codes, d_jobs + n_ring, d_slab, 0);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

int mirp_device_ensemble_reduce(mirp_ctx* c, const EnJob* d_jobs, int n_jobs, double* d_slab, const int* d_mfe, MirpEnsembleRec* d_recs, char* d_texts) {
    en_reduce_kernel<<<n_jobs, EN_NT_RED, 0, c->stream>>>(d_jobs, d_slab, d_mfe, d_recs, d_texts);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int mirp_device_ensemble_bpp(mirp_ctx* c, const EnJob* d_jobs, int n_jobs, const double* d_slab, double cutoff, int* d_row_cnt, const long long* d_row_at,
                             MirpBpp* d_out) {
    en_bpp_kernel<<<n_jobs, EN_NT_RED, 0, c->stream>>>(d_jobs, d_slab, cutoff, d_row_cnt, d_row_at, d_out);
    HIPCHK(c, hipGetLastError());
    return 0;
}

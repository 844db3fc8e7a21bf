// Differential expression between two groups (mirp_diffexp): the moments of every feature and the exact negative-binomial test
// conditioned on the feature's total n.  The host (mirp_diffexp.cpp) checks the arguments, sums the size factors, takes the median of the raw
// dispersions between de_prep_kernel and de_param_kernel and derives log2fc; everything per feature and per term runs here.
//
// The test sums u(a) = t(a) / t(k_A) over the n + 1 splits a of n: one term per read of the feature.  ln u is 0 at the observed split and is carried
// outwards from it by sums of ln rho(a), rho(a) = t(a + 1) / t(a) (de_lnrho: two divisions, two products and one log; never a difference of lgamma
// values).  So the terms of a feature are cut into chunks of C = MIRP_DIFFEXP_CHUNK *outwards from k_A*: the right side holds the terms k_A, k_A + 1,
// ..., n, the left side k_A - 1, k_A - 2, ..., 0, and chunk m of a side holds the terms at distance mC .. mC + C - 1 along it.  ln u at the start of
// a chunk is then a plain prefix of the chunk steps of its side, of the magnitude of ln u itself, and the first chunk of either side starts at 0.
//   prep    de_prep_kernel, one lane per feature: y = k / s, the three means, the pooled variance, the raw dispersion, k_A, k_B.
//   params  de_param_kernel, one lane per feature: the dispersion of the mode, r_A, r_B, pi_A / pi_B and the jobs of the feature, ceil((n - k_A + 1)
//           / C) + ceil(k_A / C) (0 for n = 0); launch_excl_scan numbers the jobs.
//   steps   de_chunk_kernel, one wave per (feature, chunk) job on a capped resident grid, wave w serving jobs w, w + waves, ...; a job finds its
//           feature by binary search over the scanned offsets.  Only a chunk with a successor on its side has work: lane l sums the steps of its
//           64 consecutive terms, de_wave_scan orders the lanes, lane 63 holds the chunk's step.  A feature below C reads has none.
//   starts  de_start_kernel, one wave per feature with a second chunk on a side: a wave scan over the chunk steps of the side, 64 at a time with a
//           carry, in place (step in, ln u at the chunk start out).
//   sums    de_sum_kernel, the same jobs: a chunk of len terms gives lane l the ceil(len / 64) consecutive terms from l * ceil(len / 64), so a
//           light feature spreads over the lanes.  The lane sums its steps, the scan gives ln u at its first term, then it walks its terms again:
//           u = exp(ln u), D += u, N += u where u <= 1 + 1e-7.  A fixed shuffle tree adds the lanes; the job's N and D go to job-indexed arrays.
//   reduce  de_reduce_kernel, one wave per feature: lane l adds the jobs l, l + 64, ... in order, the same tree adds the lanes, p = N / D.
// Every sum has a fixed order and there is no floating-point atomic: two calls on the same input give the same bytes.  The arithmetic that the
// restatement repeats bit for bit (moments, parameters, the argument of the log) is compiled without contraction into fused multiply-adds.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include "../../include/mirprefer.h"
#include "diffexp_device.h"

#pragma clang fp contract(off)

namespace mirp {

struct DeFeat {
    double ra, rb, cr;       // r_A, r_B (< 0: the Poisson case), pi_A / pi_B (Poisson: s_A / s_B)
    long long n, ka;
};

// ln rho(a), 0 <= a < n
__device__ __forceinline__ double de_lnrho(const DeFeat& f, long long a) {
    const double x = (double)a, m = (double)(f.n - a);
    double ratio = m / (x + 1.0);
    if (f.ra >= 0.0) ratio = ratio * ((x + f.ra) / ((m - 1.0) + f.rb));
    return log(ratio * f.cr);
}

// the step behind term jj of a side: right ln u(k_A + jj + 1) - ln u(k_A + jj) (none behind the last term, a = n), left ln u(k_A - 1 - jj) - ln u(k_A - jj)
__device__ __forceinline__ double de_step(const DeFeat& f, int left, long long jj) {
    if (left) return -de_lnrho(f, f.ka - 1 - jj);
    return f.ka + jj < f.n ? de_lnrho(f, f.ka + jj) : 0.0;
}

// inclusive scan over the lanes of a wave in a fixed order
__device__ __forceinline__ double de_wave_scan(double x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x;
}

// sum over the lanes of a wave in a fixed order; lane 0 holds it
__device__ __forceinline__ double de_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    return x;
}

__device__ __forceinline__ long long de_chunks(long long terms) { return (terms + DE_C - 1) / DE_C; }

__global__ void __launch_bounds__(DE_NT) de_prep_kernel(const unsigned long long* __restrict__ counts, const double* __restrict__ sf,
                                                        const unsigned char* __restrict__ group, DeConst k, double* __restrict__ q,
                                                        double* __restrict__ alpha, MirpDiffexpRow* __restrict__ rows) {
    for (long long i = (long long)blockIdx.x * DE_NT + threadIdx.x; i < k.F; i += (long long)gridDim.x * DE_NT) {
        const unsigned long long* row = counts + i * k.S;
        double sum = 0.0, sa = 0.0, sb = 0.0;
        unsigned long long ka = 0, kb = 0;
        for (int j = 0; j < k.S; j++) {
            const unsigned long long cnt = row[j];
            const double y = (double)cnt / sf[j];
            sum += y;
            if (group[j]) {
                sb += y;
                kb += cnt;
            } else {
                sa += y;
                ka += cnt;
            }
        }
        const double qi = sum / (double)k.S, qa = sa / (double)k.n_a, qb = sb / (double)k.n_b;
        double ss = 0.0;
        for (int j = 0; j < k.S; j++) {
            const int g = group[j];
            if ((g ? k.n_b : k.n_a) < 2) continue;
            const double d = (double)row[j] / sf[j] - (g ? qb : qa);
            ss += d * d;
        }
        double a = 0.0;
        if (qi > 0.0 && k.dof > 0) {
            const double v = ss / (double)k.dof, z = qi * k.mean_inv_sf;
            a = (v - z) / (qi * qi);
        }
        q[i] = qi;
        alpha[i] = a;
        MirpDiffexpRow r;
        r.base_mean = qi;
        r.mean_a = qa;
        r.mean_b = qb;
        r.log2fc = 0.0;
        r.dispersion = a;
        r.p = -1.0;
        r.k_a = ka;
        r.k_b = kb;
        rows[i] = r;
    }
}

__global__ void __launch_bounds__(DE_NT) de_param_kernel(DeConst k, int mode, double phi, double phi_c, const double* __restrict__ q,
                                                         const double* __restrict__ alpha, MirpDiffexpRow* __restrict__ rows, double* __restrict__ ra,
                                                         double* __restrict__ rb, double* __restrict__ cr, int* __restrict__ njob) {
    for (long long i = (long long)blockIdx.x * DE_NT + threadIdx.x; i < k.F; i += (long long)gridDim.x * DE_NT) {
        const double a = alpha[i];
        const double d = mode == 0 ? (a > phi_c ? a : phi_c) : mode == 1 ? phi_c : mode == 2 ? (a > 0.0 ? a : 0.0) : phi;
        const long long ka = (long long)rows[i].k_a, n = ka + (long long)rows[i].k_b;
        double xa = -1.0, xb = -1.0, c = k.s_a / k.s_b;
        if (d > 0.0 && n > 0) {                                  // n = 0 is q = 0: not tested
            const double mu_a = q[i] * k.s_a, mu_b = q[i] * k.s_b;
            xa = (k.s_a * k.s_a) / (d * k.sig_a);
            xb = (k.s_b * k.s_b) / (d * k.sig_b);
            c = (mu_a / (xa + mu_a)) / (mu_b / (xb + mu_b));
        }
        rows[i].dispersion = d;
        ra[i] = xa;
        rb[i] = xb;
        cr[i] = c;
        njob[i] = n > 0 ? (int)(de_chunks(n - ka + 1) + de_chunks(ka)) : 0;
    }
}

// the feature of job j: the last i with joff[i] <= j (a feature without jobs shares its offset with the next one and is skipped)
__device__ __forceinline__ long long de_job_feature(const long long* __restrict__ joff, long long F, long long j) {
    long long lo = 0, hi = F;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (joff[mid + 1] <= j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct DeJob {
    DeFeat f;
    int left, len;           // side; terms of the chunk, 1 .. C
    long long m, j0;         // chunk of the side, its first term along the side
    bool last;               // no chunk behind it on its side
};

__device__ __forceinline__ DeJob de_job(const long long* __restrict__ joff, long long F, long long j, const MirpDiffexpRow* __restrict__ rows,
                                        const double* __restrict__ ra, const double* __restrict__ rb, const double* __restrict__ cr) {
    const long long i = de_job_feature(joff, F, j);
    DeJob J;
    J.f.ra = ra[i];
    J.f.rb = rb[i];
    J.f.cr = cr[i];
    J.f.ka = (long long)rows[i].k_a;
    J.f.n = J.f.ka + (long long)rows[i].k_b;
    const long long R = de_chunks(J.f.n - J.f.ka + 1), local = j - joff[i];
    J.left = local >= R;
    J.m = J.left ? local - R : local;
    const long long terms = J.left ? J.f.ka : J.f.n - J.f.ka + 1;
    J.j0 = J.m * DE_C;
    J.len = (int)std::min((long long)DE_C, terms - J.j0);
    J.last = J.j0 + DE_C >= terms;
    return J;
}

__global__ void __launch_bounds__(DE_NT) de_chunk_kernel(const long long* __restrict__ joff, long long F, long long n_jobs,
                                                         const MirpDiffexpRow* __restrict__ rows, const double* __restrict__ ra,
                                                         const double* __restrict__ rb, const double* __restrict__ cr, double* __restrict__ lstep) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * DE_WAVES;
    for (long long j = (long long)blockIdx.x * DE_WAVES + (threadIdx.x >> 6); j < n_jobs; j += waves) {
        const DeJob J = de_job(joff, F, j, rows, ra, rb, cr);
        if (J.last) continue;                                        // wave-uniform; a chunk with a successor has C terms, each with a step
        double run = 0.0;
        const long long b = J.j0 + (long long)lane * (DE_C / 64);
        for (int t = 0; t < DE_C / 64; t++) run += de_step(J.f, J.left, b + t);
        run = de_wave_scan(run);
        if (lane == 63) lstep[j] = run;
    }
}

// in place: the steps of the chunks of a side -> ln u at their starts.  The last chunk of a side has no step (nothing was written there).
__global__ void __launch_bounds__(DE_NT) de_start_kernel(const long long* __restrict__ joff, const int* __restrict__ njob, long long F,
                                                         const MirpDiffexpRow* __restrict__ rows, double* __restrict__ lstep) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * DE_WAVES;
    for (long long i = (long long)blockIdx.x * DE_WAVES + (threadIdx.x >> 6); i < F; i += waves) {
        if (njob[i] == 0) continue;
        const long long ka = (long long)rows[i].k_a, n = ka + (long long)rows[i].k_b;
        const long long R = de_chunks(n - ka + 1), L = de_chunks(ka);
        if (R < 2 && L < 2) continue;
        for (int side = 0; side < 2; side++) {
            const long long cnt = side ? L : R, base = joff[i] + (side ? R : 0);
            double carry = 0.0;
            for (long long m0 = 0; m0 < cnt; m0 += 64) {             // the same trip count in every lane
                const long long m = m0 + lane;
                const double x = m < cnt - 1 ? lstep[base + m] : 0.0;
                const double incl = de_wave_scan(x);
                double excl = __shfl_up(incl, 1);
                if (lane == 0) excl = 0.0;
                if (m < cnt) lstep[base + m] = carry + excl;
                carry = carry + __shfl(incl, 63);
            }
        }
    }
}

__global__ void __launch_bounds__(DE_NT) de_sum_kernel(const long long* __restrict__ joff, long long F, long long n_jobs,
                                                       const MirpDiffexpRow* __restrict__ rows, const double* __restrict__ ra,
                                                       const double* __restrict__ rb, const double* __restrict__ cr,
                                                       const double* __restrict__ lstart, double* __restrict__ pn, double* __restrict__ pd) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * DE_WAVES;
    for (long long j = (long long)blockIdx.x * DE_WAVES + (threadIdx.x >> 6); j < n_jobs; j += waves) {
        const DeJob J = de_job(joff, F, j, rows, ra, rb, cr);
        const int T = (J.len + 63) >> 6;
        const int t0 = std::min(lane * T, J.len), t1 = std::min(t0 + T, J.len);
        double run = 0.0;
        for (int t = t0; t < t1; t++) run += de_step(J.f, J.left, J.j0 + t);
        const double incl = de_wave_scan(run);
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0.0;
        double lu = (J.m == 0 ? 0.0 : lstart[j]) + excl;             // ln u in front of the lane's first term
        double N = 0.0, D = 0.0;
        for (int t = t0; t < t1; t++) {
            const double s = de_step(J.f, J.left, J.j0 + t);
            if (J.left) lu += s;                                     // a left term lies behind its step, a right term in front of it
            const double u = exp(lu);
            if (!J.left) lu += s;
            D += u;
            if (u <= 1.0 + 1e-7) N += u;
        }
        N = de_wave_sum(N);
        D = de_wave_sum(D);
        if (lane == 0) {
            pn[j] = N;
            pd[j] = D;
        }
    }
}

__global__ void __launch_bounds__(DE_NT) de_reduce_kernel(const long long* __restrict__ joff, const int* __restrict__ njob, long long F,
                                                          const double* __restrict__ pn, const double* __restrict__ pd,
                                                          MirpDiffexpRow* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * DE_WAVES;
    for (long long i = (long long)blockIdx.x * DE_WAVES + (threadIdx.x >> 6); i < F; i += waves) {
        const long long nj = njob[i], base = joff[i];
        if (nj == 0) continue;                                       // untested: p stays -1
        double N = 0.0, D = 0.0;
        for (long long m = lane; m < nj; m += 64) {
            N += pn[base + m];
            D += pd[base + m];
        }
        N = de_wave_sum(N);
        D = de_wave_sum(D);
        if (lane == 0) rows[i].p = D > 1.7976931348623157e308 ? 0.0 : N / D;   // an overflowed denominator: p below the range of a double
    }
}

namespace {

unsigned de_grid(long long n) { return (unsigned)std::max(1ll, std::min((n + DE_NT - 1) / DE_NT, 1ll << 20)); }

// blocks of a wave-per-job launch: every job a wave of its own up to the resident cap of 4 blocks (16 waves) per CU
unsigned de_job_grid(const mirp_ctx* c, long long jobs) {
    return (unsigned)std::max(1ll, std::min((jobs + DE_WAVES - 1) / DE_WAVES, 4ll * std::max(c->n_cu, 1)));
}

}  // namespace

int de_moments(mirp_ctx* c, DeCall& D, const uint64_t* counts, const MirpDiffexpOpts* o, std::vector<double>& q, std::vector<double>& alpha) {
    const long long F = D.k.F;
    const int S = D.k.S;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    // one device allocation for the per-feature state, carved at 256-byte boundaries
    size_t need = 0;
    auto room = [&](size_t bytes) {
        const size_t at = need;
        need += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t a_counts = room(8 * (size_t)F * S), a_sf = room(8 * (size_t)S), a_group = room((size_t)S), a_q = room(8 * (size_t)F),
                 a_alpha = room(8 * (size_t)F), a_rows = room(sizeof(MirpDiffexpRow) * (size_t)F), a_ra = room(8 * (size_t)F), a_rb = room(8 * (size_t)F),
                 a_cr = room(8 * (size_t)F), a_njob = room(4 * (size_t)F), a_joff = room(8 * (size_t)(F + 1));
    char* base = (char*)D.T.get(need);
    if (!base) return fail(c, -6, "device allocation failed (diffexp)");
    D.counts = (unsigned long long*)(base + a_counts);
    D.sf = (double*)(base + a_sf);
    D.group = (unsigned char*)(base + a_group);
    D.q = (double*)(base + a_q);
    D.alpha = (double*)(base + a_alpha);
    D.rows = (MirpDiffexpRow*)(base + a_rows);
    D.ra = (double*)(base + a_ra);
    D.rb = (double*)(base + a_rb);
    D.cr = (double*)(base + a_cr);
    D.njob = (int*)(base + a_njob);
    D.joff = (long long*)(base + a_joff);
    HIPCHK(c, hipMemcpyAsync(D.counts, counts, 8 * (size_t)F * S, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(D.sf, o->size_factor, 8 * (size_t)S, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(D.group, o->group, (size_t)S, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(de_prep_kernel, dim3(de_grid(F)), dim3(DE_NT), 0, st, D.counts, D.sf, D.group, D.k, D.q, D.alpha, D.rows);
    HIPCHK(c, hipGetLastError());
    q.resize((size_t)F);
    alpha.resize((size_t)F);
    HIPCHK(c, hipMemcpyAsync(q.data(), D.q, 8 * (size_t)F, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(alpha.data(), D.alpha, 8 * (size_t)F, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return 0;
}

int de_test(mirp_ctx* c, DeCall& D, int mode, double phi, double phi_c, MirpDiffexpRow* rows, long long* jobs_out) {
    const long long F = D.k.F;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    hipLaunchKernelGGL(de_param_kernel, dim3(de_grid(F)), dim3(DE_NT), 0, st, D.k, mode, phi, phi_c, D.q, D.alpha, D.rows, D.ra, D.rb, D.cr, D.njob);
    launch_excl_scan(st, D.njob, D.joff, F);
    HIPCHK(c, hipGetLastError());
    long long jobs = 0;
    HIPCHK(c, hipMemcpyAsync(&jobs, D.joff + F, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (jobs > 0) {
        double* job3 = (double*)D.T.get(3 * 8 * (size_t)jobs);      // per job: the step / start, the partial numerator, the partial denominator
        if (!job3) return fail(c, -6, "device allocation failed (diffexp jobs)");
        double *lstep = job3, *pn = job3 + (size_t)jobs, *pd = job3 + 2 * (size_t)jobs;
        const unsigned grid = de_job_grid(c, jobs), fgrid = de_job_grid(c, F);
        hipLaunchKernelGGL(de_chunk_kernel, dim3(grid), dim3(DE_NT), 0, st, D.joff, F, jobs, D.rows, D.ra, D.rb, D.cr, lstep);
        hipLaunchKernelGGL(de_start_kernel, dim3(fgrid), dim3(DE_NT), 0, st, D.joff, D.njob, F, D.rows, lstep);
        hipLaunchKernelGGL(de_sum_kernel, dim3(grid), dim3(DE_NT), 0, st, D.joff, F, jobs, D.rows, D.ra, D.rb, D.cr, lstep, pn, pd);
        HIPCHK(c, hipGetLastError());
        c->note_jobs_per_slot(6, jobs, (long long)grid * DE_WAVES);
        hipLaunchKernelGGL(de_reduce_kernel, dim3(fgrid), dim3(DE_NT), 0, st, D.joff, D.njob, F, pn, pd, D.rows);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(rows, D.rows, sizeof(MirpDiffexpRow) * (size_t)F, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *jobs_out = jobs;
    return 0;
}

}  // namespace mirp

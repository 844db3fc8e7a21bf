// What mirp_diffexp.cpp (checks, size-factor sums, the common dispersion, log2fc) and diffexp_kernels.hip (moments and the test) share.
#pragma once
#include <cstdint>
#include <vector>
#include "mirp_ctx.h"

namespace mirp {

#define DE_C MIRP_DIFFEXP_CHUNK
#define DE_NT 256
#define DE_WAVES (DE_NT / 64)

// per-call constants of the test, all made on the host in sample order
struct DeConst {
    long long F;
    int S, n_a, n_b, dof;            // dof = the sum of n_g - 1 over the groups with two or more samples (0: no variance)
    double mean_inv_sf;              // mean of 1 / size factor
    double s_a, s_b, sig_a, sig_b;   // sums of the size factors and of their squares per group
};

// the device side of one call: its allocation lives as long as this object
struct DeCall {
    TmpDevice T;
    DeConst k;
    unsigned long long* counts = nullptr;
    double* sf = nullptr;
    unsigned char* group = nullptr;
    double *q = nullptr, *alpha = nullptr;
    MirpDiffexpRow* rows = nullptr;
    double *ra = nullptr, *rb = nullptr, *cr = nullptr;
    int* njob = nullptr;
    long long* joff = nullptr;
};

// uploads the matrix, runs de_prep_kernel (moments, raw dispersion, k_a, k_b into the device rows) and brings base_mean and the raw dispersion back
int de_moments(mirp_ctx* c, DeCall& D, const uint64_t* counts, const MirpDiffexpOpts* o, std::vector<double>& q, std::vector<double>& alpha);
// the test with the common dispersion phi_c (mode 3: unused): rows[F] on the host, the jobs of the call
int de_test(mirp_ctx* c, DeCall& D, int mode, double phi, double phi_c, MirpDiffexpRow* rows, long long* jobs);

}  // namespace mirp

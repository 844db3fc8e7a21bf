// Differential expression between two groups of samples (mirp_diffexp): the host side.  Checks every argument before a device
// allocation, sums the size factors per group in sample order, takes the common dispersion (the median of the raw dispersions that
// de_prep_kernel returns) between the two device stages and derives log2fc from the device's means.  The moments and the test are
// diffexp_kernels.hip; the size factors, the adjustment of the p-values and the files are diffexp.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mirprefer.h"
#include "diffexp_device.h"

namespace {

bool nonneg(double x) { return std::isfinite(x) && x >= 0.0; }

// median with the mean of the two middle values for an even count; v is reordered
double median_of(std::vector<double>& v) {
    const size_t n = v.size(), h = n / 2;
    std::nth_element(v.begin(), v.begin() + (long)h, v.end());
    const double hi = v[h];
    if (n & 1) return hi;
    const double lo = *std::max_element(v.begin(), v.begin() + (long)h);
    return (lo + hi) / 2.0;
}

}  // namespace

extern "C" int mirp_diffexp(mirp_ctx* c, const uint64_t* counts, int64_t n_features, const MirpDiffexpOpts* o, MirpDiffexpRow** rows, int64_t stats[5]) {
    using namespace mirp;
    if (!c) return -1;
    if (!o || !rows || !o->size_factor || !o->group || (n_features > 0 && !counts)) return fail(c, -1, "mirp_diffexp: bad argument");
    if (n_features < 0 || n_features > MIRP_DIFFEXP_MAX_FEATURES) return fail(c, -1, "mirp_diffexp: n_features outside 0 .. 2^24");
    if (o->n_samples < 2 || o->n_samples > MIRP_MAX_SAMPLES) return fail(c, -1, "mirp_diffexp: n_samples outside 2 .. 255");
    if (o->mode < 0 || o->mode > 3) return fail(c, -1, "mirp_diffexp: mode outside 0 .. 3");
    if (!nonneg(o->phi) || !nonneg(o->min_mean) || !nonneg(o->pseudo)) return fail(c, -1, "mirp_diffexp: phi, min_mean and pseudo must be finite and >= 0");
    const long long F = n_features;
    const int S = o->n_samples;
    DeCall D;
    DeConst& k = D.k;
    k.F = F;
    k.S = S;
    k.n_a = k.n_b = 0;
    k.s_a = k.s_b = k.sig_a = k.sig_b = 0.0;
    double inv = 0.0;
    for (int j = 0; j < S; j++) {
        const double s = o->size_factor[j];
        if (!(std::isfinite(s) && s > 0.0)) return fail(c, -1, "mirp_diffexp: size factor " + std::to_string(j + 1) + " is not finite and > 0");
        if (o->group[j] > 1) return fail(c, -1, "mirp_diffexp: group " + std::to_string(j + 1) + " is neither 0 nor 1");
        inv += 1.0 / s;
        if (o->group[j]) {
            k.n_b++;
            k.s_b += s;
            k.sig_b += s * s;
        } else {
            k.n_a++;
            k.s_a += s;
            k.sig_a += s * s;
        }
    }
    k.mean_inv_sf = inv / (double)S;
    if (k.n_a == 0 || k.n_b == 0) return fail(c, -1, "mirp_diffexp: a group without a sample");
    k.dof = (k.n_a >= 2 ? k.n_a - 1 : 0) + (k.n_b >= 2 ? k.n_b - 1 : 0);
    if (o->mode != 3 && k.dof == 0) return fail(c, -1, "mirp_diffexp: modes 0 .. 2 need a group of two or more samples");
    long long terms = 0, tested = 0;
    for (long long i = 0; i < F; i++) {
        unsigned long long n = 0;
        for (int j = 0; j < S; j++) {
            const uint64_t v = counts[(size_t)i * S + j];
            if (v >= (uint64_t)MIRP_DIFFEXP_MAX_COUNT) return fail(c, -1, "mirp_diffexp: feature " + std::to_string(i + 1) + " has a count of 2^40 or more");
            n += v;
        }
        if (n > 0) {
            tested++;
            terms += (long long)n + 1;
            if (terms > (long long)MIRP_DIFFEXP_MAX_COUNT) return fail(c, -1, "mirp_diffexp: more than 2^40 terms");
        }
    }
    *rows = nullptr;
    c->reset_jobs_per_slot(6);
    MirpDiffexpRow* h_rows = (MirpDiffexpRow*)std::calloc((size_t)std::max(F, 1ll), sizeof(MirpDiffexpRow));
    if (!h_rows) return fail(c, -6, "host allocation failed (diffexp)");
    long long jobs = 0;
    double phi_c = o->mode == 3 ? o->phi : 0.0;
    if (F > 0) {
        std::vector<double> q, alpha;
        int rc = de_moments(c, D, counts, o, q, alpha);
        if (!rc && o->mode != 3) {
            std::vector<double> kept;
            for (long long i = 0; i < F; i++)
                if (q[(size_t)i] >= o->min_mean) kept.push_back(alpha[(size_t)i]);
            if (!kept.empty()) phi_c = std::max(0.0, median_of(kept));
            else if (o->mode != 2) rc = fail(c, -10, "mirp_diffexp: no feature has a mean of min_mean or more, so there is no common dispersion");
        }
        if (!rc) rc = de_test(c, D, o->mode, o->phi, phi_c, h_rows, &jobs);
        if (rc) {
            std::free(h_rows);
            return rc;
        }
        for (long long i = 0; i < F; i++) h_rows[i].log2fc = std::log2((h_rows[i].mean_b + o->pseudo) / (h_rows[i].mean_a + o->pseudo));
    }
    *rows = h_rows;
    if (stats) {
        stats[0] = F;
        stats[1] = tested;
        stats[2] = jobs;
        stats[3] = terms;
        std::memcpy(&stats[4], &phi_c, 8);
    }
    return 0;
}

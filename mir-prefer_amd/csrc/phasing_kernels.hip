// Phased-siRNA (PHAS) window scan on the context's resident alignments (mirp_phase_scan).  The host (phasing.py) turns alpha into
// the kmin table, merges the passing windows into loci and writes the files; everything per record, per unit and per anchor runs here.
//
// The resident records are sorted by (tid, pos).  A record of length L is one read of the unit (tid, strand, c), c = pos on the plus strand and
// pos + 2 on the minus strand, held as the 64-bit key tid << 32 | c (c < 2^32: pos < 2^31).  The records of one strand, taken in order, are
// already sorted by key, so the units need no sort:
//   split    ph_flag_kernel: length L on + / on -; two launch_excl_scan; ph_gather_kernel packs the keys and depths, the + stream, then the - stream.
//   units    ph_head_kernel: a key that differs from its predecessor (or starts a stream) starts a unit; launch_excl_scan numbers them;
//            ph_unit_kernel sums the depths per unit (64-bit atomics) and keeps its key.
//   -d       ph_keep_kernel + launch_excl_scan + ph_compact_kernel: the units with abundance >= D.  The abundance is split into its low 30 bits and
//            the rest, and the two int32 scans (launch_excl_scan) give exact 64-bit prefix sums P, so a range of units sums in O(1).
//   anchors  ph_merge_kernel: the merge path of the two sorted unit streams (+ before - on equal keys); every merged entry keeps its lower bound in
//            both streams.  The first entry of each key is an anchor.
//   scan     ph_window_kernel<0>, one lane per merged entry (adjacent lanes search adjacent units).  Per strand, n is the distance from the anchor's
//            lower bound to the lower bound of x + mL, searched over at most mL units; k counts the phased coordinates x + jL present, each found by
//            a binary search over at most L units that starts where the previous one stopped (the keys are distinct integers).  That is O(m log L)
//            per anchor, also when every coordinate is taken.  A window passes when k >= max(kmin[n], K); launch_excl_scan of the pass flags;
//            ph_window_kernel<1> recomputes the passing anchors with their abundance sums and writes them in (tid, start) order.
// split, units and -d are ph_build_units, which the trigger scan (trigger_kernels.hip, §29) calls as well; the searches and the counting of one
// strand are in phasing_units.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "mirp_ctx.h"
#include "phasing_units.h"

namespace mirp {

#define PH_NT 256

static inline unsigned ph_grid(long long n) { return (unsigned)std::max(1ll, std::min((n + PH_NT - 1) / PH_NT, 1ll << 20)); }

__global__ void __launch_bounds__(PH_NT) ph_flag_kernel(const MirpAln* __restrict__ a, long long n, int L, int* __restrict__ fp, int* __restrict__ fm) {
    for (long long i = (long long)blockIdx.x * PH_NT + threadIdx.x; i < n; i += (long long)gridDim.x * PH_NT) {
        const MirpAln r = a[i];
        const bool ok = r.len == L && r.pos >= 0;
        fp[i] = ok && !r.strand;
        fm[i] = ok && r.strand;
    }
}

__global__ void __launch_bounds__(PH_NT) ph_gather_kernel(const MirpAln* __restrict__ a, long long n, int L, const long long* __restrict__ sp,
                                                          const long long* __restrict__ sm, long long np, unsigned long long* __restrict__ key,
                                                          unsigned* __restrict__ dep) {
    for (long long i = (long long)blockIdx.x * PH_NT + threadIdx.x; i < n; i += (long long)gridDim.x * PH_NT) {
        const MirpAln r = a[i];
        if (r.len != L || r.pos < 0) continue;
        const long long j = r.strand ? np + sm[i] : sp[i];
        key[j] = ((unsigned long long)(unsigned)r.tid << 32) + (unsigned long long)r.pos + (r.strand ? 2ull : 0ull);
        dep[j] = r.depth;
    }
}

__global__ void __launch_bounds__(PH_NT) ph_head_kernel(const unsigned long long* __restrict__ key, long long n, long long np, int* __restrict__ head) {
    for (long long j = (long long)blockIdx.x * PH_NT + threadIdx.x; j < n; j += (long long)gridDim.x * PH_NT)
        head[j] = j == 0 || j == np || key[j] != key[j - 1];
}

__global__ void __launch_bounds__(PH_NT) ph_unit_kernel(const unsigned long long* __restrict__ key, const unsigned* __restrict__ dep,
                                                        const int* __restrict__ head, const long long* __restrict__ us, long long n,
                                                        unsigned long long* __restrict__ ab, unsigned long long* __restrict__ ukey) {
    for (long long j = (long long)blockIdx.x * PH_NT + threadIdx.x; j < n; j += (long long)gridDim.x * PH_NT) {
        const int h = head[j];
        const long long u = us[j] + h - 1;
        atomicAdd(&ab[u], (unsigned long long)dep[j]);
        if (h) ukey[u] = key[j];
    }
}

__global__ void __launch_bounds__(PH_NT) ph_keep_kernel(const unsigned long long* __restrict__ ab, long long n, unsigned long long min_depth,
                                                        int* __restrict__ keep) {
    for (long long u = (long long)blockIdx.x * PH_NT + threadIdx.x; u < n; u += (long long)gridDim.x * PH_NT) keep[u] = ab[u] >= min_depth;
}

__global__ void __launch_bounds__(PH_NT) ph_compact_kernel(const unsigned long long* __restrict__ ukey, const unsigned long long* __restrict__ ab,
                                                           const int* __restrict__ keep, const long long* __restrict__ ks, long long n,
                                                           unsigned long long* __restrict__ fkey, int* __restrict__ lo, int* __restrict__ hi) {
    for (long long u = (long long)blockIdx.x * PH_NT + threadIdx.x; u < n; u += (long long)gridDim.x * PH_NT) {
        if (!keep[u]) continue;
        const long long v = ks[u];
        const unsigned long long x = ab[u];        // < 2^61 (2^29 records x 2^32 - 1 at most): the high part fits an int
        fkey[v] = ukey[u];
        lo[v] = (int)(x & 0x3fffffffull);
        hi[v] = (int)(x >> 30);
    }
}

__global__ void __launch_bounds__(PH_NT) ph_merge_kernel(const unsigned long long* __restrict__ fkey, long long np, long long n,
                                                         unsigned long long* __restrict__ mkey, longlong2* __restrict__ mlb) {
    for (long long v = (long long)blockIdx.x * PH_NT + threadIdx.x; v < n; v += (long long)gridDim.x * PH_NT) {
        const unsigned long long k = fkey[v];
        long long r;
        longlong2 b;
        if (v < np) {
            b.x = v;
            b.y = ph_lower(fkey + np, 0, n - np, k);
            r = v + b.y;
        } else {
            b.x = ph_upper(fkey, 0, np, k);        // = the lower bound whenever this entry is an anchor (no plus unit with its key)
            b.y = v - np;
            r = b.y + b.x;
        }
        mkey[r] = k;
        mlb[r] = b;
    }
}

template <int EMIT>
__global__ void __launch_bounds__(PH_NT) ph_window_kernel(const unsigned long long* __restrict__ mkey, const longlong2* __restrict__ mlb, PhUnits U,
                                                          int L, int m, int min_phased, const int* __restrict__ kmin, int* __restrict__ pass,
                                                          const long long* __restrict__ pscan, MirpPhaseWindow* __restrict__ out,
                                                          unsigned long long* __restrict__ n_anchors) {
    const long long n = U.n;
    for (long long base = (long long)blockIdx.x * PH_NT; base < n; base += (long long)gridDim.x * PH_NT) {
        const long long r = base + threadIdx.x;
        bool anchor = false;
        if (r < n) {
            if (EMIT) anchor = pass[r] != 0;
            else anchor = r == 0 || mkey[r - 1] != mkey[r];
        }
        if (!EMIT) {
            const unsigned long long b = __ballot(anchor);
            if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_anchors, (unsigned long long)__popcll(b));
        }
        if (!anchor) {
            if (!EMIT && r < n) pass[r] = 0;
            continue;
        }
        const unsigned long long x = mkey[r];
        const longlong2 lb = mlb[r];
        int nn = 0, kk = 0;
        long long phased = 0, reads = 0;
        ph_strand<EMIT>(U, lb.x, U.np, x, L, m, nn, kk, phased, reads);
        ph_strand<EMIT>(U, U.np + lb.y, n, x, L, m, nn, kk, phased, reads);
        if (!EMIT) {
            pass[r] = kk >= max(kmin[nn], min_phased);
        } else {
            MirpPhaseWindow w;
            w.tid = (int)(x >> 32);
            w.n = nn;
            w.k = kk;
            w.reserved = 0;
            w.start = (long long)(x & 0xffffffffull);
            w.phased_reads = phased;
            w.window_reads = reads;
            out[pscan[r]] = w;
        }
    }
}

}  // namespace mirp

namespace {

int ph_count(mirp_ctx* c, const long long* d, long long* h) {
    HIPCHK(c, hipMemcpyAsync(h, d, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

int mirp::ph_build_units(mirp_ctx* c, int L, int min_depth, TmpDevice& T, PhUnits* U, long long* records) {
    using namespace mirp;
    const hipStream_t st = c->stream;
    const long long n = c->n_alns;
    const MirpAln* alns = (const MirpAln*)c->alns.p;
    long long rec_p = 0, rec_m = 0, nk = 0;
    long long *sp = nullptr, *sm = nullptr;
    *U = PhUnits{nullptr, nullptr, nullptr, 0, 0};
    *records = 0;
    auto grab = [&](size_t bytes) { return T.get(bytes); };
    if (n > 0) {
        int* fp = (int*)grab(4 * (size_t)n);
        int* fm = (int*)grab(4 * (size_t)n);
        sp = (long long*)grab(8 * (size_t)(n + 1));
        sm = (long long*)grab(8 * (size_t)(n + 1));
        if (!fp || !fm || !sp || !sm) return fail(c, -6, "device allocation failed (phase scan)");
        hipLaunchKernelGGL(ph_flag_kernel, dim3(ph_grid(n)), dim3(PH_NT), 0, st, alns, n, L, fp, fm);
        launch_excl_scan(st, fp, sp, n);
        launch_excl_scan(st, fm, sm, n);
        HIPCHK(c, hipGetLastError());
        if (int rc = ph_count(c, sp + n, &rec_p)) return rc;
        if (int rc = ph_count(c, sm + n, &rec_m)) return rc;
    }
    const long long nrec = rec_p + rec_m;
    *records = nrec;
    if (nrec == 0) return 0;
    unsigned long long* key = (unsigned long long*)grab(8 * (size_t)nrec);
    unsigned* dep = (unsigned*)grab(4 * (size_t)nrec);
    int* head = (int*)grab(4 * (size_t)nrec);
    long long* us = (long long*)grab(8 * (size_t)(nrec + 1));
    if (!key || !dep || !head || !us) return fail(c, -6, "device allocation failed (phase scan)");
    hipLaunchKernelGGL(ph_gather_kernel, dim3(ph_grid(n)), dim3(PH_NT), 0, st, alns, n, L, sp, sm, rec_p, key, dep);
    hipLaunchKernelGGL(ph_head_kernel, dim3(ph_grid(nrec)), dim3(PH_NT), 0, st, key, nrec, rec_p, head);
    launch_excl_scan(st, head, us, nrec);
    HIPCHK(c, hipGetLastError());
    long long nu = 0, nu_p = 0;
    if (int rc = ph_count(c, us + nrec, &nu)) return rc;
    if (int rc = ph_count(c, us + rec_p, &nu_p)) return rc;
    unsigned long long* ab = (unsigned long long*)grab(8 * (size_t)nu);
    unsigned long long* ukey = (unsigned long long*)grab(8 * (size_t)nu);
    int* keep = (int*)grab(4 * (size_t)nu);
    long long* ks = (long long*)grab(8 * (size_t)(nu + 1));
    if (!ab || !ukey || !keep || !ks) return fail(c, -6, "device allocation failed (phase scan)");
    HIPCHK(c, hipMemsetAsync(ab, 0, 8 * (size_t)nu, st));
    hipLaunchKernelGGL(ph_unit_kernel, dim3(ph_grid(nrec)), dim3(PH_NT), 0, st, key, dep, head, us, nrec, ab, ukey);
    hipLaunchKernelGGL(ph_keep_kernel, dim3(ph_grid(nu)), dim3(PH_NT), 0, st, ab, nu, (unsigned long long)min_depth, keep);
    launch_excl_scan(st, keep, ks, nu);
    HIPCHK(c, hipGetLastError());
    long long nk_p = 0;
    if (int rc = ph_count(c, ks + nu, &nk)) return rc;
    if (int rc = ph_count(c, ks + nu_p, &nk_p)) return rc;
    if (nk == 0) return 0;
    unsigned long long* fkey = (unsigned long long*)grab(8 * (size_t)nk);
    int* lo = (int*)grab(4 * (size_t)nk);
    int* hi = (int*)grab(4 * (size_t)nk);
    long long* slo = (long long*)grab(8 * (size_t)(nk + 1));
    long long* shi = (long long*)grab(8 * (size_t)(nk + 1));
    if (!fkey || !lo || !hi || !slo || !shi) return fail(c, -6, "device allocation failed (phase scan)");
    hipLaunchKernelGGL(ph_compact_kernel, dim3(ph_grid(nu)), dim3(PH_NT), 0, st, ukey, ab, keep, ks, nu, fkey, lo, hi);
    launch_excl_scan(st, lo, slo, nk);
    launch_excl_scan(st, hi, shi, nk);
    HIPCHK(c, hipGetLastError());
    *U = PhUnits{fkey, slo, shi, nk_p, nk};
    return 0;
}

extern "C" int mirp_phase_scan(mirp_ctx* c, const MirpPhaseOpts* o, const int32_t* kmin, MirpPhaseWindow** windows, int64_t* n_windows, int64_t stats[3]) {
    using namespace mirp;
    if (!c) return -1;
    if (!o || !kmin || !windows || !n_windows) return fail(c, -1, "mirp_phase_scan: bad argument");
    if (o->length < 1 || o->length > 1024 || o->cycles < 1 || o->cycles > 64 || o->min_phased < 1 || o->min_depth < 1)
        return fail(c, -1, "mirp_phase_scan: bad options");
    *windows = nullptr;
    *n_windows = 0;
    HIPCHK(c, hipSetDevice(c->device));
    const int L = o->length, m = o->cycles, S = 2 * m * L;
    const hipStream_t st = c->stream;
    long long nrec = 0, nw = 0;
    unsigned long long anchors = 0;
    TmpDevice T;
    MirpPhaseWindow* d_out = nullptr;
    PhUnits U;
    auto grab = [&](size_t bytes) { return T.get(bytes); };
    if (int rc = ph_build_units(c, L, o->min_depth, T, &U, &nrec)) return rc;
    const long long nk = U.n;
    if (nk > 0) {
        unsigned long long* mkey = (unsigned long long*)grab(8 * (size_t)nk);
        longlong2* mlb = (longlong2*)grab(16 * (size_t)nk);
        int* pass = (int*)grab(4 * (size_t)nk);
        long long* pscan = (long long*)grab(8 * (size_t)(nk + 1));
        int* d_kmin = (int*)grab(4 * (size_t)(S + 1));
        unsigned long long* d_anchors = (unsigned long long*)grab(8);
        if (!mkey || !mlb || !pass || !pscan || !d_kmin || !d_anchors) return fail(c, -6, "device allocation failed (phase scan)");
        HIPCHK(c, hipMemcpyAsync(d_kmin, kmin, 4 * (size_t)(S + 1), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemsetAsync(d_anchors, 0, 8, st));
        hipLaunchKernelGGL(ph_merge_kernel, dim3(ph_grid(nk)), dim3(PH_NT), 0, st, U.key, U.np, nk, mkey, mlb);
        hipLaunchKernelGGL(ph_window_kernel<0>, dim3(ph_grid(nk)), dim3(PH_NT), 0, st, mkey, mlb, U, L, m, (int)o->min_phased, d_kmin, pass,
                           (const long long*)nullptr, (MirpPhaseWindow*)nullptr, d_anchors);
        launch_excl_scan(st, pass, pscan, nk);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&anchors, d_anchors, 8, hipMemcpyDeviceToHost, st));
        if (int rc = ph_count(c, pscan + nk, &nw)) return rc;
        if (nw > 0) {
            d_out = (MirpPhaseWindow*)grab(sizeof(MirpPhaseWindow) * (size_t)nw);
            if (!d_out) return fail(c, -6, "device allocation failed (phase scan)");
            hipLaunchKernelGGL(ph_window_kernel<1>, dim3(ph_grid(nk)), dim3(PH_NT), 0, st, mkey, mlb, U, L, m, (int)o->min_phased, d_kmin, pass,
                               pscan, d_out, d_anchors);
            HIPCHK(c, hipGetLastError());
        }
    }
    MirpPhaseWindow* h_out = (MirpPhaseWindow*)std::malloc(sizeof(MirpPhaseWindow) * (size_t)std::max(nw, 1ll));
    if (!h_out) return fail(c, -6, "host allocation failed (phase scan)");
    if (nw > 0) {
        const hipError_t e1 = hipMemcpyAsync(h_out, d_out, sizeof(MirpPhaseWindow) * (size_t)nw, hipMemcpyDeviceToHost, st);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamSynchronize(st) : e1;
        if (e2 != hipSuccess) {
            std::free(h_out);
            return fail(c, -2, std::string("mirp_phase_scan: ") + hipGetErrorString(e2));
        }
    }
    *windows = h_out;
    *n_windows = nw;
    if (stats) {
        stats[0] = nrec;
        stats[1] = nk;
        stats[2] = (long long)anchors;
    }
    return 0;
}

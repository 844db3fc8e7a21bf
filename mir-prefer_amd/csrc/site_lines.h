// The back half of the (miRNA, bin) site searches (targets_kernels.hip, mimic_kernels.hip): from the keys of one pass to text,
// and the plan of the passes when the keys of a search overflow the buffer.  A search supplies its line as a functor
//     struct Line { <text tables>; static constexpr int shift; template <bool WRITE> __device__ long long line(key, idx, out) const; };
// shift = the key bits below the miRNA index, line() = the length of the line of sorted key `idx` of the pass, written to `out` with WRITE.
//
//   order  mirp_device_sort_u64 by the whole key = the output order.
//   cut    site_size_kernel: the line's length, 0 where -k cuts the key (site_kept, site_keys.h); site_emitted_kernel; launch_excl_scan.
//   emit   site_emit_kernel writes the lines; the text goes to the sink in pieces of whole lines, at most c->text_piece_bytes() each (1 GiB
//          unless a test lowered it; text_pieces.h), counted in c->text_pieces.
// The keys, offsets and text of a pass live in the context's tg_* buffers, which both searches size.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <string>
#include <vector>
#include "mirp_ctx.h"
#include "pass_plan.h"
#include "site_keys.h"
#include "text_pieces.h"

namespace mirp {

// size[i] of sorted key i, 0 when -k cuts it (emitted[key >> shift] = lines of the miRNA written by earlier passes); kept[0] += lines kept
template <class LINE>
__global__ void site_size_kernel(LINE line, const unsigned long long* __restrict__ keys, long long n, long long k, const unsigned long long* __restrict__ emitted,
                                 int* __restrict__ size, unsigned long long* __restrict__ kept) {
    unsigned long long cnt = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const bool keep = site_kept(keys, i, k, emitted, LINE::shift);
        size[i] = keep ? (int)line.template line<false>(keys[i], i, nullptr) : 0;
        cnt += keep;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(kept, cnt);
}
// emitted[key >> SHIFT] += the miRNA's keys in this pass (after site_size_kernel)
template <int SHIFT>
__global__ void site_emitted_kernel(const unsigned long long* __restrict__ keys, long long n, unsigned long long* __restrict__ emitted) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        if (i == n - 1 || (keys[i + 1] >> SHIFT) != (keys[i] >> SHIFT)) emitted[keys[i] >> SHIFT] += (unsigned long long)(i + 1 - site_run_first(keys, i, SHIFT));
}
template <class LINE>
__global__ void site_emit_kernel(LINE line, const unsigned long long* __restrict__ keys, long long i0, long long i1, const long long* __restrict__ toff,
                                 char* __restrict__ text) {
    const long long base = toff[i0];
    for (long long i = i0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < i1; i += (long long)gridDim.x * blockDim.x)
        if (toff[i + 1] != toff[i]) (void)line.template line<true>(keys[i], i, text + (toff[i] - base));
}

inline int site_grid(long long n) {
    const long long g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > 16384 ? 16384 : g);
}

struct SiteNoStep { int operator()(const unsigned long long*, long long) const { return 0; } };

// Sorts, cuts and writes the n <= cap keys of a pass in tg_keys.  key_bits: the key's bits in use (the higher ones are 0); max_sites: -k, 0 = all;
// before_sizes(d_keys, n): runs on the sorted keys before the lines are measured and sees tg_emitted as the earlier passes left it; name: the
// search, for the allocation message.  stats = {sites written, passes}; sec[1] += sort and cut, sec[2] += emit, download and sink.
template <class LINE, class Step = SiteNoStep>
int site_finish_pass(mirp_ctx* c, const LINE& line, long long n, int key_bits, long long max_sites, const std::function<int(const char*, size_t)>& sink,
                     const char* name, long long stats[2], double sec[3], Step before_sizes = Step()) {
    hipStream_t st = c->stream;
    stats[1]++;
    if (n == 0) return 0;
    double t = now();
    const unsigned long long* d_keys = (const unsigned long long*)c->tg_keys.p;
    if (int rc = mirp_device_sort_u64(c, (unsigned long long*)c->tg_keys.p, (unsigned long long*)c->tg_ktmp.p, n, 0, (key_bits + 7) / 8 * 8)) return rc;
    unsigned long long* d_kept = (unsigned long long*)c->tg_small.p + 1;
    unsigned long long* d_emitted = (unsigned long long*)c->tg_emitted.p;
    const long long* d_toff = (const long long*)c->tg_toff.p;
    HIPCHK(c, hipMemsetAsync(d_kept, 0, 8, st));
    if (int rc = before_sizes(d_keys, n)) return rc;
    hipLaunchKernelGGL(site_size_kernel<LINE>, dim3(site_grid(n)), dim3(256), 0, st, line, d_keys, n, max_sites, (const unsigned long long*)d_emitted,
                       (int*)c->tg_size.p, d_kept);
    hipLaunchKernelGGL(site_emitted_kernel<LINE::shift>, dim3(site_grid(n)), dim3(256), 0, st, d_keys, n, d_emitted);
    launch_excl_scan(st, (const int*)c->tg_size.p, (long long*)c->tg_toff.p, n);
    long long bytes = 0;
    unsigned long long kept = 0;
    HIPCHK(c, hipMemcpyAsync(&bytes, d_toff + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&kept, d_kept, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    stats[0] += (long long)kept;
    sec[1] += now() - t;
    t = now();
    const auto read_toff = [&](long long i, long long* v) -> int {
        HIPCHK(c, hipMemcpy(v, d_toff + i, 8, hipMemcpyDeviceToHost));
        return 0;
    };
    for (long long i0 = 0, base = 0; i0 < n;) {
        long long i1 = n, end = bytes;
        if (int rc = text_piece_end(i0, n, base, bytes, c->text_piece_bytes(), read_toff, &i1, &end)) return rc;
        const long long len = end - base;
        if (len > 0) {
            if (c->tg_text.ensure((size_t)len + 16)) return fail(c, -6, std::string("device allocation failed (") + name + ": text)");
            hipLaunchKernelGGL(site_emit_kernel<LINE>, dim3(site_grid(i1 - i0)), dim3(256), 0, st, line, d_keys, i0, i1, d_toff, (char*)c->tg_text.p);
            HIPCHK(c, hipStreamSynchronize(st));
            HIPCHK(c, hipGetLastError());
            if (c->h_text.size() < (size_t)len) c->h_text.resize((size_t)len);
            HIPCHK(c, hipMemcpy(c->h_text.data(), c->tg_text.p, (size_t)len, hipMemcpyDeviceToHost));
            c->text_pieces++;
            if (int rc = sink(c->h_text.data(), (size_t)len)) return rc;
        }
        i0 = i1;
        base = end;
    }
    sec[2] += now() - t;
    return 0;
}

// The passes of a search whose first scan found more than `cap` keys (pass_plan.h).  The bins are (miRNA, b), b < nbin, numbered in
// output order; a miRNA takes part in a scan with the bins lo .. hi of its range.
//   scan(mode, ma, mb, p0, p1, &got)   miRNAs ma .. mb at positions [p0, p1) of [0, total) with the ranges as set; mode 1 counts the hits per bin
//                                      into tg_hist (n_mi * nbin counters), mode 0 leaves the keys in tg_keys; got = hits (maybe > cap)
//   set_range(m, lo, hi)               lo > hi closes the range: every range is closed except during the scan of a pass that holds the miRNA
//   finish(got)                        sorts, cuts and writes the got <= cap keys of the last scan
// top: the highest bin in use; max_sites: -k, under which no pass goes past the bin at which a miRNA's first k lines are reached.  name and
// over_cap word the two errors of a plan.
template <class SetRange, class Scan, class Finish>
int site_plan_passes(mirp_ctx* c, long long n_mi, int nbin, int top, long long max_sites, long long cap, unsigned long long total, const char* name,
                     const char* over_cap, SetRange set_range, Scan scan, Finish finish) {
    HIPCHK(c, hipMemsetAsync(c->tg_hist.p, 0, 8 * (size_t)n_mi * nbin, c->stream));
    long long hits = 0;
    if (int rc = scan(1, 0ll, n_mi - 1, 0ull, total, &hits)) return rc;
    std::vector<unsigned long long> hist((size_t)n_mi * nbin);
    HIPCHK(c, hipMemcpy(hist.data(), c->tg_hist.p, 8 * hist.size(), hipMemcpyDeviceToHost));
    std::vector<int> lim((size_t)n_mi, top);
    if (max_sites > 0)
        for (long long m = 0; m < n_mi; m++) {
            unsigned long long cum = 0;
            for (int h = 0; h <= top; h++) {
                cum += hist[(size_t)m * nbin + h];
                if (cum >= (unsigned long long)max_sites) { lim[(size_t)m] = h; break; }
            }
        }
    const auto close = [&](long long ma, long long mb) { for (long long m = ma; m <= mb; m++) set_range(m, 1, 0); };
    close(0, n_mi - 1);
    const auto count = [&](long long i) { return (int)(i % nbin) <= lim[(size_t)(i / nbin)] ? (long long)hist[(size_t)i] : 0ll; };
    const auto flush = [&](long long first, long long last, long long expected) -> int {
        const long long ma = first / nbin, mb = last / nbin;
        const int ha = (int)(first % nbin), hb = (int)(last % nbin);
        for (long long m = ma; m <= mb; m++) set_range(m, m == ma ? ha : 0, m == mb ? hb : lim[(size_t)m]);
        long long got = 0;
        const int rc = scan(0, ma, mb, 0ull, total, &got);
        close(ma, mb);
        if (rc) return rc;
        if (got != expected) return fail(c, -5, std::string(name) + ": a pass found a different number of sites than counted");
        return finish(got);
    };
    const auto range = [&](long long bin, unsigned long long p, unsigned long long p1, long long* got) -> int {
        const long long m = bin / nbin;
        const int h = (int)(bin % nbin);
        set_range(m, h, h);
        const int rc = scan(0, m, m, p, p1, got);
        close(m, m);
        if (rc) return rc;
        return *got > cap ? 0 : finish(*got);
    };
    const int rc = plan_passes(n_mi * nbin, count, cap, total, flush, range);
    return rc == PLAN_POSITION_OVER_CAP ? fail(c, -5, over_cap) : rc;
}

}  // namespace mirp

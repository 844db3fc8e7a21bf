// Device-side text writer shared by the kernels that format output lines (align_kernels.hip, targets_kernels.hip, mimic_kernels.hip): the same
// routine first measures a line (WRITE = false, nothing is stored) and then writes it at its scanned offset (WRITE = true).  The lines of the site
// searches share their head and their pairing block (text_site_head, text_site_pairing); a search adds its score and its trailing columns.
#pragma once
#include <hip/hip_runtime.h>
#include "site_keys.h"

namespace mirp {

__device__ __forceinline__ int text_digits(unsigned long long v) { int d = 1; while (v >= 10) { v /= 10; d++; } return d; }

template <bool WRITE>
struct TextOut {
    char* p;
    long long n = 0;
    __device__ void ch(char c) { if (WRITE) p[n] = c; n++; }
    __device__ void num(unsigned long long v) {
        const int d = text_digits(v);
        if (WRITE) for (int k = d - 1; k >= 0; k--) { p[n + k] = (char)('0' + v % 10); v /= 10; }
        n += d;
    }
    __device__ void str(const char* s, long long len) { if (WRITE) for (long long k = 0; k < len; k++) p[n + k] = s[k]; n += len; }
    __device__ void lit(const char* s) { while (*s) ch(*s++); }
};

// the head of a site's line: miRNA m, target a, the interval's 1-based start and end in the target, strand (names as blobs with offsets)
template <bool WRITE>
__device__ void text_site_head(TextOut<WRITE>& o, const char* mnames, const long long* mnoff, long long m, const char* tnames, const long long* tnoff, int a,
                               unsigned long long start, unsigned long long end, int strand) {
    o.str(mnames + mnoff[m], mnoff[m + 1] - mnoff[m]);
    o.ch('\t');
    o.str(tnames + tnoff[a], tnoff[a + 1] - tnoff[a]);
    o.ch('\t');
    o.num(start);
    o.ch('\t');
    o.num(end);
    o.ch('\t');
    o.ch(strand ? '-' : '+');
}

// the pairing block of a site's line: mismatches gu mirna_5to3 pairs target_3to5.  Column c = 1 .. W of the three aligned strings holds miRNA
// position pos(c) (0 = none; mc: the miRNA's codes, 0..3 = A C G U, 4 = unknown) over the target-strand base base(c) (0..3, below 0 = none); a
// column that lacks either is no pair and shows '-' in its place and under `pairs`.
template <bool WRITE, class Pos, class Base>
__device__ void text_site_pairing(TextOut<WRITE>& o, const unsigned char* mc, int W, Pos pos, Base base) {
    const char* RNA = "ACGUN";
    auto cls = [&](int c) {
        const int i = pos(c), y = base(c);
        return i == 0 || y < 0 ? 3 : site_class(mc[i - 1], (unsigned)y);
    };
    int nmm = 0, ngu = 0;
    for (int c = 1; c <= W; c++) {
        const int k = cls(c);
        nmm += k == 2;
        ngu += k == 1;
    }
    o.num((unsigned long long)nmm);
    o.ch('\t');
    o.num((unsigned long long)ngu);
    o.ch('\t');
    for (int c = 1; c <= W; c++) { const int i = pos(c); o.ch(i ? RNA[mc[i - 1]] : '-'); }
    o.ch('\t');
    for (int c = 1; c <= W; c++) { const int k = cls(c); o.ch(k == 0 ? '|' : k == 1 ? 'o' : k == 2 ? 'x' : '-'); }
    o.ch('\t');
    for (int c = 1; c <= W; c++) { const int y = base(c); o.ch(y < 0 ? '-' : RNA[y]); }
}

}  // namespace mirp

// Device-side text writer shared by the kernels that format output lines (align_kernels.hip, targets_kernels.hip): the same routine first
// measures a line (WRITE = false, nothing is stored) and then writes it at its scanned offset (WRITE = true).
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace mirp

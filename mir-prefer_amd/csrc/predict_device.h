// What predict_kernel.hip and homolog_kernels.hip share on the device: the structure rules (ss_words.h: the structure list of a window, a8, MP:1541-1724,
// and get_maturestar_info with its duplex rules, a9, MP:1727-1999), the structure record and the stager of the dot-bracket text.
#pragma once
#include <hip/hip_runtime.h>
#include "ss_words.h"

namespace mirp {

// One structure piece of a window: line index, offset and length inside the line, kind (0 stem-loop, 1 good bifurcation).
// start and normalised energy are recomputed from the line record.
struct PStruct { unsigned short line, off, len, type; };

// Dot-bracket text staged in LDS as two 1-bit planes ('(' and ')'), one 64-bit word per 32 characters (ss_words.h): a window's lines then take <= 9 KB
// instead of 34 KB, which is what bounds the number of resident windows per CU.
// Word wi of a line whose text starts at p and has ss_stride bytes (a multiple of 4 is read in full; the rest of the last four is left clear).
__device__ __forceinline__ unsigned long long d_stage_word(const char* __restrict__ p, int ss_stride, int wi) {
    const int lim = ss_stride - wi * 32;       // bytes of this line left
    p += wi * 32;
    unsigned op = 0, cl = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        unsigned four = 0;
        if (q * 4 + 4 <= lim) four = *reinterpret_cast<const unsigned*>(p + q * 4);
        ssw_pack4(four, q * 4, op, cl);
    }
    return ssw_word(op, cl);
}

}  // namespace mirp

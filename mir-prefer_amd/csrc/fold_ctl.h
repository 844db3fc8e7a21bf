// The control block of the LDS-resident fold (c->fctl): 32-bit words that the kernels of fold_lds_kernel.hip count in and the driver (mirp_fold.cpp)
// clears and reads.  Block 0 belongs to the call, block 1 + k to chunk k of a chunked fold; the serial path uses block 0 alone, for every sub-batch.
// A kernel is handed pointers to single words (its work counter, the fallback count, the dense list's length) and reaches their neighbours through the
// differences of these names.  Host and device.
#pragma once

namespace mirp {

enum : int {
    FOLD_CTL_FILL = 0,          // work counter of the candidate-pool pass, or of a dense pass over every window
    FOLD_CTL_EPILOGUE = 1,      // work counter of the epilogue
    FOLD_CTL_DENSE = 2,         // work counter of the dense pass over the dense list
    FOLD_CTL_DENSE_LEN = 3,     // windows a pool pass handed to the dense pass: the length of the dense list
    FOLD_CTL_FALLBACKS = 4,     // block 0 only: windows handed to the generic kernel (the length of the fallback list), over the whole call
    FOLD_CTL_DENSE_TOTAL = 5,   // running total of FOLD_CTL_DENSE_LEN over the dense passes that used the block (mirp_last_fold_dense)
    FOLD_CTL_POOL_MAX = 6,      // block 0 only: largest fill of a candidate pool, over the whole call
    // block 0 only, written by fold_dup_count_kernel when mirp_fold skips duplicate windows (fold dedup): they reach the host with the block
    FOLD_CTL_DUP_FALLBACKS = 7, // duplicates of the windows on the fallback list
    FOLD_CTL_DUP_DENSE = 8,     // duplicates of the windows the dense passes took
    FOLD_CTL_DUPLICATES = 9,    // duplicates among the call's windows
    FOLD_CTL_BLOCK = 16,        // words of a block
    FOLD_CTL_CLOCKS = 16,       // diagnostics build, serial path: FOLD_CTL_CLOCKS_N 64-bit clocks from this word on (over blocks the serial path has no use for)
    FOLD_CTL_CLOCKS_N = 4 + 64 + 8 + 3 + 16,
    FOLD_CTL_MIN_BYTES = 1024   // the driver allocates and clears at least this much
};
static_assert(4 * FOLD_CTL_CLOCKS % 8 == 0 && 4 * FOLD_CTL_CLOCKS + 8 * FOLD_CTL_CLOCKS_N <= FOLD_CTL_MIN_BYTES, "the diagnostics clocks lie inside what the driver clears");
static_assert(FOLD_CTL_DUPLICATES < FOLD_CTL_CLOCKS &&FOLD_CTL_CLOCKS <= FOLD_CTL_BLOCK, "the clocks leave the words of block 0 alone");

}  // namespace mirp

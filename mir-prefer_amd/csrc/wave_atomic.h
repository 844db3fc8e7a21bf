// Integer atomics on per-group accumulators, one per distinct address of a wave: a hotspot group costs one atomic per wave, no lane loops over
// its members, and the results do not depend on scheduling (clusters_kernels.hip, degradome_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace mirp {

// OP 0: a[slot] += v, 1: a[slot] = max, 2: a[slot] = min, for every lane with slot >= 0.  Every lane of the wave must call it.  One atomic per
// distinct slot of the wave (at most 64 rounds); the value of each slot is reduced across its lanes first.
template <int OP>
__device__ __forceinline__ void cl_wave_atomic(unsigned long long* __restrict__ a, long long slot, unsigned long long v) {
    const int lane = threadIdx.x & 63;
    bool todo = slot >= 0;
    while (true) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const long long s = __shfl(slot, leader);
        const bool mine = todo && slot == s;
        unsigned long long x = mine ? v : (OP == 2 ? ~0ull : 0ull);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(x, o);
            x = OP == 0 ? x + y : OP == 1 ? (x > y ? x : y) : (x < y ? x : y);
        }
        if (lane == leader) {
            if (OP == 0) atomicAdd(&a[s], x);
            else if (OP == 1) atomicMax(&a[s], x);
            else atomicMin(&a[s], x);
        }
        if (mine) todo = false;
    }
}

// a[slot] += 1 on 32-bit counters, for every lane with slot >= 0 (libqc_kernels.hip).  Every lane of the wave must call it.  One atomic per distinct
// slot of the wave: the lanes of a slot are counted by a ballot, so nothing is reduced.
__device__ __forceinline__ void cl_wave_count32(unsigned* __restrict__ a, int slot) {
    const int lane = threadIdx.x & 63;
    bool todo = slot >= 0;
    while (true) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const int s = __shfl(slot, leader);
        const bool mine = todo && slot == s;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&a[s], (unsigned)__popcll(same));
        if (mine) todo = false;
    }
}

}  // namespace mirp

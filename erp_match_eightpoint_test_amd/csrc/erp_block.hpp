// erp_block.hpp -- the wave and block prefix scans every kernel file shares (device).
#pragma once

#include <hip/hip_runtime.h>

namespace erp {

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ int wave_inclusive_scan(int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// exclusive scan over a block of BLOCK threads (BLOCK multiple of 64, <= 1024); ws holds
// BLOCK / 64 ints; every thread of the block calls it, and it ends past a barrier
template <int BLOCK>
__device__ int block_exclusive_scan(int v, int* ws, int* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // (the wave scan written out: through wave_inclusive_scan the compiler schedules the
    // consensus and matcher kernels differently, and their code is to stay as it is)
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) ws[wid] = x;
    __syncthreads();
    if (wid == 0) {
        int t = lane < BLOCK / 64 ? ws[lane] : 0;
#pragma unroll
        for (int o = 1; o < BLOCK / 64; o <<= 1) {
            const int y = __shfl_up(t, o, 64);
            if (lane >= o) t += y;
        }
        if (lane < BLOCK / 64) ws[lane] = t;
    }
    __syncthreads();
    const int base = wid ? ws[wid - 1] : 0;
    *total = ws[BLOCK / 64 - 1];
    __syncthreads();
    return base + x - v;
}

}  // namespace erp

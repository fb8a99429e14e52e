// erp_winner.hpp -- which iteration pushed row min_idx (device; shared by polish.hip and
// winner.hip).  Rows are pushed R1 then R2 per record, in iteration order
// (src/eight_point.cpp:113-126), so the row's owner follows from a prefix sum over the
// iterations' validity flags.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/erp_match.h"

namespace erp {

constexpr int kWinnerThreads = 256;
constexpr int kWinnerWaves = kWinnerThreads / 64;

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ int winner_wave_scan(int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// From the hypothesis records' two validity flags: a block prefix scan over 256-record chunks
// (the strided read of the 120-B records stops at the chunk that holds the winner).  Every
// thread of the kWinnerThreads-thread block calls it; win[0] = the iteration (-1: min_idx names
// no row of these records), win[1] = 0 for its R1, 1 for its R2; ends past a barrier.
__device__ inline void winner_from_records(const erp_hypothesis* hyps, int iters, int min_idx,
                                           int* wsum, int* win) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) win[0] = -1;
    __syncthreads();
    int base = 0;
    for (int h0 = 0; h0 < iters; h0 += kWinnerThreads) {
        const int h = h0 + tid;
        int v1 = 0, c = 0;
        if (h < iters) {
            v1 = hyps[h].R1_valid != 0;
            c = v1 + (hyps[h].R2_valid != 0);
        }
        const int x = winner_wave_scan(c, lane);
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWinnerWaves; w++) {
            wbase += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
        const int first = base + wbase + x - c;  // the row this record's first rotation got
        if (c && min_idx >= first && min_idx < first + c) {
            win[0] = h;
            win[1] = (v1 && min_idx == first) ? 0 : 1;
        }
        base += total;
        __syncthreads();
        if (win[0] >= 0 || base > min_idx) break;
    }
}

}  // namespace erp

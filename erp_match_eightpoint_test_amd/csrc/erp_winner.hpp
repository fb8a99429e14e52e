// erp_winner.hpp -- which iteration pushed row min_idx (device; shared by polish.hip and
// winner.hip).  Rows are pushed R1 then R2 per record, in iteration order
// (src/eight_point.cpp:113-126), so the row's owner follows from a prefix sum over the
// iterations' validity flags.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/erp_match.h"
#include "erp_block.hpp"

namespace erp {

constexpr int kWinnerThreads = 256;
constexpr int kWinnerWaves = kWinnerThreads / 64;

// From the hypothesis records' two validity flags: a block prefix scan over 256-record chunks
// (the strided read of the 120-B records stops at the chunk that holds the winner).  Every
// thread of the kWinnerThreads-thread block calls it; win[0] = the iteration (-1: min_idx names
// no row of these records), win[1] = 0 for its R1, 1 for its R2; ends past a barrier.
__device__ inline void winner_from_records(const erp_hypothesis* hyps, int iters, int min_idx,
                                           int* wsum, int* win) {
    const int tid = threadIdx.x;
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
        int total;
        // the row this record's first rotation got
        const int first = base + block_exclusive_scan<kWinnerThreads>(c, wsum, &total);
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

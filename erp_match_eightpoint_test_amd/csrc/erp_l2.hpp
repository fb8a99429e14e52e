// erp_l2.hpp -- the exact descriptor distance and the k=2 update every matcher kernel shares
// (matcher.hip's rescore and sweep kernels, guided.hip's gated rematch): one definition, so a
// distance computed by either stage has the same bits.
#pragma once

#include <hip/hip_runtime.h>

namespace erp {

// exact squared distance in the flann::L2<float> order: per group of 4,
// acc += d0*d0 + d1*d1 + d2*d2 + d3*d3 (no FMA)
__device__ __forceinline__ float exact_l2(const float4* qr, const float4* __restrict__ tp) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const float4 tv = tp[c];
        const float d0 = qr[c].x - tv.x;
        const float d1 = qr[c].y - tv.y;
        const float d2 = qr[c].z - tv.z;
        const float d3 = qr[c].w - tv.w;
        acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    return acc;
}

// k=2 update with the sweep's tie rule (lowest train index first among equal distances)
__device__ __forceinline__ void top2_consider(float acc, int j, float& b0, int& j0, float& b1) {
    if (acc < b0 || (acc == b0 && j < j0)) {
        b1 = b0;
        b0 = acc;
        j0 = j;
    } else if (acc < b1) {
        b1 = acc;
    }
}

}  // namespace erp

// erp_jump_poly.hpp -- the one-wave polynomial product of the glibc jump-ahead, shared by
// kernels.hip (jump_prep_kernel) and rand_stream.hip (the rand stream's kernels).
//
// glibc TYPE_3: r[n+31] = r[n+28] + r[n] (mod 2^32), so x^d mod P(x) = x^31 - x^28 - 1 maps a
// 31-word window r[n..n+30] to r[n+d..n+d+30].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace erp {

// One wave: out = a * b mod P (31 coefficients each, in LDS).  Lane n < 61 forms the
// convolution coefficient c_n; lanes t < 31 then fold c_31..c_60 with the reduction table
// column they hold in registers (cred[d] = x^(31+d) mod P, coefficient t).  out may alias
// neither a nor b.
__device__ __forceinline__ void pmul_wave(const uint32_t* a, const uint32_t* b, uint32_t* out,
                                          const uint32_t (&cred)[30]) {
    const int lane = threadIdx.x & 63;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 31; i++) {
        const int j = lane - i;
        const uint32_t bj = (j >= 0 && j <= 30) ? b[j < 0 ? 0 : (j > 30 ? 30 : j)] : 0u;
        c += a[i] * bj;
    }
    uint32_t r = c;
#pragma unroll
    for (int d = 0; d < 30; d++) r += (uint32_t)__builtin_amdgcn_readlane((int)c, 31 + d) * cred[d];
    if (lane < 31) out[lane] = r;
}

}  // namespace erp

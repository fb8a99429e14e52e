// winner.hip -- the winner stage (include/erp_match.h "winner records"; no reference
// counterpart): the essential matrix of the iteration the consensus chose, without the
// per-iteration hypothesis records.  It runs behind the consensus and only reads what the run
// left in the context's scratch; capi.hip's run_winners hands it the pointers.
//
// One workgroup of 256 threads per pair, one launch:
//   locate    the iteration and the rotation (R1 / R2) that pushed row min_idx: from the records'
//             validity flags when the run wrote records (erp_winner.hpp), else from the lite
//             estimates -- wave 0 scans the per-64-iteration valid counts (wsum[p][w][0]) to the
//             wave that holds the row, then that wave's 64 NaN-x marks (hl[p][0][h], hl[p][3][h]).
//   gram      the threads stride over the pair's rows; a row whose bit is set in the winner
//             iteration's selection words (word b, bit u <-> row M-1-31b-u; pair rep[p]'s words
//             when the launch shared replays) adds its 36 values q = rint((LL RR) 2^44) -- what
//             gram_limbs_kernel cuts into int8 digits -- into per-thread int64 sums.  The block
//             adds them up: integers, so any order gives the MFMA kernel's sum.
//   solve     lane 0: the sums to fp64 with the one rounding gram_join makes, then the
//             pipeline's three-way path (s < 9: gram36_to_full + gram_jacobi9; else
//             gram_min_eigvec9_inv, gram_min_eigvec9_jacobi where it does not settle) -- the
//             same device functions under the same -ffp-contract=off, so the same bits.
//   check     lane 0: estimate_from_e on that E; the chosen rotation must be valid and it and T
//             must equal the result record's R, T byte for byte, else ERP_INTERNAL and zeros.
// A latency-bound fp64 kernel like polish_kernel: no MFMA, no atomics, nothing per draw.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/erp_match.h"
#include "erp_device.hpp"
#include "erp_kernels.hpp"
#include "erp_launch.hpp"
#include "erp_stage.hpp"
#include "erp_winner.hpp"

namespace erp {

namespace {

constexpr double kWinnerGramScale = 0x1p44;  // gram_limbs_kernel's fixed point (kGramScale)

// the pair's record when it has no winner: the status and zeros
__device__ void winner_none(const WinnerArgs& a, int p, int32_t status) {
    if (threadIdx.x == 0) a.out[p] = stage_record<erp_winner>(status);
}

// the lite route's locate (wave 0 only): win as winner_from_records leaves it
__device__ void winner_from_lite(const float* hl, const int32_t* vw, int iters, int nwaves,
                                 int min_idx, int* win) {
    const int lane = threadIdx.x & 63;
    int base = 0, ww = -1, wfirst = 0;
    for (int w0 = 0; w0 < nwaves; w0 += 64) {  // (every bound below is wave-uniform)
        const int w = w0 + lane;
        const int c = w < nwaves ? vw[(size_t)w * 8] : 0;
        const int x = wave_inclusive_scan(c, lane);
        const int first = base + x - c;  // the row the wave's first valid rotation got
        const uint64_t hit = __ballot(c > 0 && min_idx >= first && min_idx < first + c);
        if (hit) {
            const int src = __ffsll((unsigned long long)hit) - 1;
            ww = w0 + src;
            wfirst = __shfl(first, src, 64);
            break;
        }
        base += __shfl(x, 63, 64);
        if (base > min_idx) break;
    }
    if (ww < 0) return;
    const int h = ww * 64 + lane;
    int v1 = 0, c = 0;
    if (h < iters) {
        v1 = !__builtin_isnan(hl[h]);
        c = v1 + !__builtin_isnan(hl[(size_t)3 * iters + h]);
    }
    const int x = wave_inclusive_scan(c, lane);
    const int first = wfirst + x - c;
    if (c && min_idx >= first && min_idx < first + c) {
        win[0] = h;
        win[1] = (v1 && min_idx == first) ? 0 : 1;
    }
}

__global__ __launch_bounds__(kWinnerThreads) void winner_kernel(WinnerArgs a) {
    __shared__ long long red[36][kWinnerWaves];
    __shared__ int wsum[kWinnerWaves];
    __shared__ int win[2];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const erp_pair_result* res = a.results + p;
    if (res->status != ERP_OK) {  // (block-uniform, as every early return below)
        winner_none(a, p, res->status);
        return;
    }
    const int iters = a.iters, min_idx = res->min_idx;
    const int M = a.counts[p];
    const int s = (int)(M * a.sample_frac);
    if (M < 1 || M > a.max_nq || s < 1) {  // not what an ERP_OK pair of this run looks like
        winner_none(a, p, ERP_INTERNAL);
        return;
    }

    // ---- locate ----
    if (a.hyps) {
        winner_from_records(a.hyps + (size_t)p * iters, iters, min_idx, wsum, win);
    } else {
        if (tid == 0) win[0] = -1;
        __syncthreads();
        if (wave == 0)
            winner_from_lite(a.hl + (size_t)p * 9 * iters, a.wsum + (size_t)p * a.nwaves * 8,
                             iters, a.nwaves, min_idx, win);
        __syncthreads();
    }
    const int winner = win[0], which = win[1];
    if (winner < 0 || winner >= iters) {  // min_idx names no row
        winner_none(a, p, ERP_INTERNAL);
        return;
    }

    // ---- the winner iteration's Gram, as exact integer sums ----
    const int ps = a.rep ? a.rep[p] : p;  // the words' owner (sampler_alias_kernel)
    const uint32_t* sp = a.selw + (((size_t)ps * a.nwaves + (winner >> 6)) * (size_t)a.nbw) * 64 +
                         (winner & 63);
    const double* P = a.pts + (size_t)p * (a.max_nq + 1) * 6;
    long long g[36];
#pragma unroll
    for (int k = 0; k < 36; k++) g[k] = 0;
    int n = 0;
    for (int i = tid; i < M; i += kWinnerThreads) {
        const int k = M - 1 - i, b = k / 31, u = k - 31 * b;  // (b <= (M-1)/31 < nbw)
        if (!((sp[(size_t)b * 64] >> u) & 1u)) continue;
        n++;
        const double* pr = P + (size_t)i * 6;
        const double l0 = pr[0], l1 = pr[1], l2 = pr[2], r0 = pr[3], r1 = pr[4], r2 = pr[5];
        // (l l^T) and (r r^T) index pairs 00 01 02 11 12 22, entry 6 a + e = LL[a] RR[e]
        const double LL[6] = {l0 * l0, l0 * l1, l0 * l2, l1 * l1, l1 * l2, l2 * l2};
        const double RR[6] = {r0 * r0, r0 * r1, r0 * r2, r1 * r1, r1 * r2, r2 * r2};
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
            for (int e = 0; e < 6; e++)
                g[6 * c + e] += __double2ll_rn((LL[c] * RR[e]) * kWinnerGramScale);
    }
#pragma unroll
    for (int k = 0; k < 36; k++) {
        long long v = g[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[k][wave] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (tid != 0) return;

    // ---- solve and check (one lane) ----
    double g36[36];
    for (int k = 0; k < 36; k++) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < kWinnerWaves; w++) v += red[k][w];
        // v 2^-44 rounded once, as gram_join rounds its limb sums: hi 2^24 + lo with both parts
        // exact in fp64 (|hi| < 2^40, 0 <= lo < 2^24), one fma
        const long long hi = v >> 24, lo = v - hi * (1ll << 24);
        g36[k] = __builtin_fma((double)hi, 0x1p-20, (double)lo * 0x1p-44);
    }
    int rows = 0;
#pragma unroll
    for (int w = 0; w < kWinnerWaves; w++) rows += wsum[w];
    double e[9];
    if (s < 9) {
        double G[81];
        gram36_to_full(g36, G);
        gram_jacobi9(G, s, e);
    } else if (!gram_min_eigvec9_inv(g36, 1, 0, e)) {
        gram_min_eigvec9_jacobi(g36, 1, 0, e);
    }
    Hyp hy;
    estimate_from_e(e, a.valid_abs, hy);
    const float* R = which ? hy.R2 : hy.R1;
    bool same = (which ? hy.R2_valid : hy.R1_valid) != 0 && rows == s;
#pragma unroll
    for (int k = 0; k < 3; k++)
        same = same && __float_as_uint(R[k]) == __float_as_uint(res->R[k]) &&
               __float_as_uint(hy.T[k]) == __float_as_uint(res->T[k]);
    erp_winner o = stage_record<erp_winner>(same ? ERP_OK : ERP_INTERNAL);
    if (same) {
        o.iter = winner;
        o.which = which;
        o.sample_n = rows;
#pragma unroll
        for (int k = 0; k < 9; k++) o.E[k] = e[k];
    }
    a.out[p] = o;
}

}  // namespace

hipError_t launch_winner(const WinnerArgs& a, int n_pairs, hipStream_t st) {
    ERP_LAUNCH(winner_kernel, dim3((unsigned)n_pairs), dim3(kWinnerThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace erp

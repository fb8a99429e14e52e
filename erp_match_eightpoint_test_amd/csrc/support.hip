// support.hip -- the support stage (include/erp_match.h "support-scored winner"; no reference
// counterpart): per pair, every iteration's inlier count under |l^T E' r| < thr and the scored
// iteration with the largest count, behind the consensus and from what the run left in the
// context's scratch; capi.hip's run_support hands it the pointers.  Its launches:
//   prep     one lane per iteration: e_h -- the record's E, or on the lite route evec[p][9][h]
//            with estimate_lite_kernel<true>'s three-way rule applied again from the HBM Gram
//            (s < 9: gram36_to_full + gram_jacobi9; e[0] NaN: gram_min_eigvec9_jacobi; the same
//            device functions on the same operands under the same -ffp-contract=off, so the
//            same bits) -- then E'_h = rank2_correct(e_h) as fp64 [p][iters][9] (the exact path)
//            and as the count kernel's operand image.
//   points   one lane per match: u = l (x) r in the count kernel's operand image.
//   count    count_h = #{i < M : |l_i^T E'_h r_i| < thr} into counts[p][iters], exactly: a fast
//            evaluation decides every residual further than d from thr, the rest is redone in
//            fp64 with inlier_residual.  Two forms of the fast evaluation (ERP_OPT_SUPPORT_COUNT):
//            the f32 VALU chain of kernels.hip's inlier_count_kernel, and bf16 MFMA (below).
//   select   one workgroup per pair: the first argmax over the scored iterations, `which`,
//            `row`, the consensus iteration and its count, a self-check of the chosen iteration
//            (estimate_from_e on e_iter must give the run's validity marks and, byte for byte,
//            the rotation and T it stored, else ERP_INTERNAL and zeros), and the records.
//
// The MFMA count.  Per pair the residuals are the product (M x 9) (9 x iters).  Both factors are
// split into two bf16 terms, x = xh + xm + xr with xh = bf16(x), xm = bf16(x - xh) (x - xh is
// exact in fp64), |xr| <= (2^-9 + 2^-24)^2 |x| < 2^-18 (1 + 2^-13) |x| (round to nearest even,
// done here in integer arithmetic; the 2^-24 is the fp64 -> f32 step before it).  The products
// kept lie along K of v_mfma_f32_32x32x16_bf16, two MFMAs per 32 x 32 tile:
//   k = 0..8  uh_k E'h_k     k = 9..17  uh_k E'm_k     k = 18..26  um_k E'h_k     k = 27..31  0
// Dropped: um E'm + uh E'r + ur E'h + (terms of order 2^-27), in sum over k at most
//   3 2^-18 (1 + 2^-12) sum_k |u_k| |E'_k| <= 3 2^-18 (1 + 2^-12) ||u|| ||E'||_F = 1.1446e-5,
// with ||u|| = |l| |r| = 1 (pixel_to_bearing's unit vectors, up to ulps) and ||E'||_F <= ||e|| = 1
// (rank2_correct drops a singular value of a unit vector's matrix) -- the prep checks the latter
// per iteration and takes an iteration with ||E'||_F^2 > 1 + 2^-20, or a non-finite E', out of
// the fast path altogether (its count is then a plain fp64 loop).  Every bf16 x bf16 product is
// exact in f32; the accumulation of the 27 products (and 5 zeros) into the f32 accumulator, in
// whatever order and with whatever rounding direction the matrix core applies per addition, adds
// at most 32 additions x 2^-23 (twice the round-to-nearest bound: truncation allowed) x the
// largest partial sum, which is <= sum |terms| <= (1 + 2^-7) ||u|| ||E'||_F: < 3.85e-6.  The
// fp64 reference chain itself is within 10 2^-53 of the real-number product.  Together
//   |acc - res64| < 1.1446e-5 + 3.85e-6 + 1e-15 < 1.53e-5,
// and d = 2^-15 = 3.0518e-5, twice that, is taken.  The compared constants are lo = the f32
// below (thr - d) and hi = the f32 above (thr + d), so that their own rounding only widens the
// band.  The bf16 operands are finite, so no accumulator is NaN.  |acc| < lo counts the match,
// |acc| >= hi does not, and the lanes that hold the rest redo them with inlier_residual on the
// fp64 bearings and the fp64 E'.  Rows >= M of the last tile are masked by their index and
// iterations >= iters are never stored.  The VALU form keeps inlier_count_kernel's derivation
// (d = 2^-19 for the f32 chain).
//
// Layout of the MFMA kernel: A = 32 matches x 16 k (LDS, staged 256 matches at a time through
// registers so the next stage's global loads fly during the tiles), B = 16 k x 32 iterations
// (registers, held for the whole pair), C/D = 32 x 32 with the iteration on the lane (col = lane
// & 31) and 16 matches in the registers (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)): a lane's 16
// values all belong to its iteration, so the count is a per-lane add and the only cross-lane
// step is the final add of the two lane halves.  A wave owns 32 iterations, a block of 4 waves
// 128.  LDS: 16 KB.  No atomics, no packed FP32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/erp_match.h"
#include "erp_block.hpp"
#include "erp_device.hpp"
#include "erp_kernels.hpp"
#include "erp_launch.hpp"
#include "erp_stage.hpp"
#include "erp_winner.hpp"

namespace erp {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float kVBand = 0x1p-19f;       // the f32 chain's d (kernels.hip kInlierBand)
constexpr double kMBand = 0x1p-15;       // the MFMA form's d (file header)
constexpr double kNormMax = 1.0 + 0x1p-20;
constexpr int kVChunk = 256;             // matches per pass of a VALU wave (4 per lane)
constexpr int kSelThreads = kWinnerThreads;
constexpr int kSelWaves = kSelThreads / 64;

// bf16 bits of x rounded to nearest even (finite x)
__device__ __forceinline__ uint32_t bf16_bits(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_value(uint32_t bits) { return __uint_as_float(bits << 16); }

// x = hi + mid + (a remainder below 2^-18 |x|): the two bf16 terms' bits
__device__ __forceinline__ void split_bf16(double x, uint32_t* hi, uint32_t* mid) {
    *hi = bf16_bits((float)x);
    *mid = bf16_bits((float)(x - (double)bf16_value(*hi)));
}

// whether pair p runs: its result status (block-uniform)
__device__ __forceinline__ bool pair_runs(const SupportArgs& a, int p) {
    return a.results[p].status == ERP_OK;
}

// e_h of pair p: the record's E, or the lite route's three-way rule (file header)
__device__ __forceinline__ void solved_e(const SupportArgs& a, int p, int h, int s, double* e) {
    const int iters = a.iters;
    if (a.hyps) {
        const erp_hypothesis* hy = a.hyps + (size_t)p * iters + h;
#pragma unroll
        for (int k = 0; k < 9; k++) e[k] = hy->E[k];
        return;
    }
    const double* ei = a.evec + (size_t)p * 9 * iters + h;
    const double* gi = a.gram + (size_t)p * 36 * iters + h;
#pragma unroll
    for (int k = 0; k < 9; k++) e[k] = ei[(size_t)k * iters];
    if (s < 9) {
        double g36[36], G[81];
#pragma unroll
        for (int k = 0; k < 36; k++) g36[k] = gi[(size_t)k * iters];
        gram36_to_full(g36, G);
        gram_jacobi9(G, s, e);
    } else if (__builtin_isnan(e[0])) {
        gram_min_eigvec9_jacobi(gi, iters, 0, e);
    }
}

// ------------------------------------------------------------------------------ prep ----
// Two instantiations, as estimate_lite_kernel: REST = false takes the iterations whose e_h is
// stored (the records route, and the lite route's settled lanes of pairs with s >= 9) and is not
// sized by the Jacobi paths' live doubles; REST = true (lite route only) takes the others.
template <bool REST>
__global__ __launch_bounds__(64) void support_prep_kernel(SupportArgs a) {
    const int p = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
    if (!pair_runs(a, p) || h >= a.ipad) return;
    uint32_t* img = (uint32_t*)a.eimg + ((size_t)p * a.ipad + h) * 16;  // 64 B per iteration
    if (h >= a.iters) {  // the MFMA form's padding columns: zero operands, never stored
        if (a.mfma && !REST) {
#pragma unroll
            for (int k = 0; k < 16; k++) img[k] = 0;
            a.xflag[(size_t)p * a.ipad + h] = 0;
        }
        return;
    }
    const int s = (int)(a.mcount[p] * a.sample_frac);
    double e[9], Ec[9];
    if (REST) {
        if (s >= 9 && !__builtin_isnan(a.evec[(size_t)p * 9 * a.iters + h])) return;
        solved_e(a, p, h, s, e);
    } else if (a.hyps) {
        const erp_hypothesis* hy = a.hyps + (size_t)p * a.iters + h;
#pragma unroll
        for (int k = 0; k < 9; k++) e[k] = hy->E[k];
    } else {
        if (s < 9) return;  // (the whole pair is the other instantiation's)
        const double* ei = a.evec + (size_t)p * 9 * a.iters + h;
#pragma unroll
        for (int k = 0; k < 9; k++) e[k] = ei[(size_t)k * a.iters];
        if (__builtin_isnan(e[0])) return;
    }
    rank2_correct(e, Ec);
    double* o = a.ec64 + ((size_t)p * a.iters + h) * 9;
    double n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        o[k] = Ec[k];
        n2 += Ec[k] * Ec[k];
    }
    if (!a.mfma) {  // the f32 image [16]: 9 values, the rest unused
#pragma unroll
        for (int k = 0; k < 9; k++) img[k] = __float_as_uint((float)Ec[k]);
        return;
    }
    // the B operand's 32 bf16 along K (file header); an iteration outside the bound's
    // assumptions gets zeros and the flag: the count kernel counts it in fp64
    const bool fast = n2 <= kNormMax;  // (false for NaN)
    uint16_t b[32];
#pragma unroll
    for (int k = 0; k < 32; k++) b[k] = 0;
    if (fast) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            uint32_t hi, mid;
            split_bf16(Ec[k], &hi, &mid);
            b[k] = (uint16_t)hi;
            b[9 + k] = (uint16_t)mid;
            b[18 + k] = (uint16_t)hi;
        }
    }
#pragma unroll
    for (int k = 0; k < 16; k++) img[k] = (uint32_t)b[2 * k] | ((uint32_t)b[2 * k + 1] << 16);
    a.xflag[(size_t)p * a.ipad + h] = fast ? 0 : 1;
}

// ---------------------------------------------------------------------------- points ----
// VALU form: u = fl(l) (x) fl(r) as f32, SoA [p][9][mpad], rows >= M NaN (never counted);
// MFMA form: the A operand's 32 bf16 along K per match, [p][mpad][32], rows >= M zero
__global__ __launch_bounds__(256) void support_points_kernel(SupportArgs a) {
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (!pair_runs(a, p) || i >= a.mpad) return;
    const int M = min(a.mcount[p], a.max_nq);
    const double* q = a.pts + ((size_t)p * (a.max_nq + 1) + i) * 6;
    if (!a.mfma) {
        float* o = (float*)a.uimg + (size_t)p * 9 * a.mpad + i;
        if (i >= M) {
#pragma unroll
            for (int k = 0; k < 9; k++) o[(size_t)k * a.mpad] = __builtin_nanf("");
            return;
        }
        const float l[3] = {(float)q[0], (float)q[1], (float)q[2]};
        const float r[3] = {(float)q[3], (float)q[4], (float)q[5]};
#pragma unroll
        for (int k = 0; k < 9; k++) o[(size_t)k * a.mpad] = l[k / 3] * r[k % 3];
        return;
    }
    uint32_t* img = (uint32_t*)a.uimg + ((size_t)p * a.mpad + i) * 16;
    uint16_t b[32];
#pragma unroll
    for (int k = 0; k < 32; k++) b[k] = 0;
    if (i < M) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            uint32_t hi, mid;
            split_bf16(q[k / 3] * q[3 + k % 3], &hi, &mid);
            b[k] = (uint16_t)hi;
            b[9 + k] = (uint16_t)hi;
            b[18 + k] = (uint16_t)mid;
        }
    }
#pragma unroll
    for (int k = 0; k < 16; k++) img[k] = (uint32_t)b[2 * k] | ((uint32_t)b[2 * k + 1] << 16);
}

// the exact residual test of match i under iteration h of pair p
__device__ __forceinline__ bool exact_inlier(const SupportArgs& a, int p, int h, int i) {
    const double* E64 = a.ec64 + ((size_t)p * a.iters + h) * 9;
    const double* b = a.pts + ((size_t)p * (a.max_nq + 1) + i) * 6;
    return fabs(inlier_residual(E64, b, b + 3)) < a.thr;
}

// ------------------------------------------------------------------------ count, VALU ----
// kernels.hip inlier_count_kernel's technique on the prep's E': one wave per 64 iterations of a
// pair, 256 matches in VGPRs, E' wave-uniform, the count of a (chunk, iteration) on the SALU.
__global__ __launch_bounds__(64) void support_count_valu_kernel(SupportArgs a) {
    const int p = blockIdx.y, lane = threadIdx.x, h0 = blockIdx.x * 64;
    const int iters = a.iters;
    const int nh = min(64, iters - h0);
    int32_t* out = a.counts + (size_t)p * iters + h0;
    if (!pair_runs(a, p)) {  // a pair that does not run: a row of zeros
        if (lane < nh) out[lane] = 0;
        return;
    }
    const int M = min(a.mcount[p], a.max_nq), mpad = a.mpad;
    const float* U = (const float*)a.uimg + (size_t)p * 9 * mpad;
    const float* E32 = (const float*)a.eimg + ((size_t)p * a.ipad + h0) * 16;
    const float thr_lo = a.thr_lo, thr_hi = a.thr_hi;
    int acc = 0;
    for (int c0 = 0; c0 < M; c0 += kVChunk) {
        float u[4][9];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int k = 0; k < 9; k++) u[q][k] = U[(size_t)k * mpad + c0 + q * 64 + lane];
        for (int h = 0; h < nh; h++) {
            const float* e = E32 + h * 16;
            float ev[9];
#pragma unroll
            for (int k = 0; k < 9; k++) ev[k] = e[k];
            int cnt = 0;
            uint64_t amb_any = 0;
            bool amb[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float res = ev[0] * u[q][0];
#pragma unroll
                for (int k = 1; k < 9; k++) res = fmaf(ev[k], u[q][k], res);
                const float v = fabsf(res);
                const uint64_t in = __ballot(v < thr_lo);
                const uint64_t below_hi = __ballot(v < thr_hi);
                cnt += __popcll(in);
                amb[q] = ((below_hi & ~in) >> lane) & 1;
                amb_any |= below_hi & ~in;
            }
            if (amb_any) {  // rare: the matches the f32 value cannot decide, exactly
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool ex = amb[q] && exact_inlier(a, p, h0 + h, c0 + q * 64 + lane);
                    cnt += __popcll(__ballot(ex));
                }
            }
            acc = lane == h ? acc + cnt : acc;
        }
    }
    if (lane < nh) out[lane] = acc;
}

// ------------------------------------------------------------------------ count, MFMA ----
constexpr int kMTile = 32;                     // matches per MFMA tile
constexpr int kMStage = 256;                   // matches per LDS stage (8 tiles)
constexpr int kMWaveIters = 32, kMBlockIters = 128, kMThreads = 256;

// the tile's epilogue: acc holds 16 matches (rows) of the lane's iteration.  TAIL: rows >= M
// exist in the tile.  Returns the matches counted.
template <bool TAIL>
__device__ __forceinline__ int support_epilogue(const SupportArgs& a, const f32x16& acc, int p, int h,
                                                bool h_ok, int row0, int M, float lo, float hi) {
    int cnt = 0;
    bool amb = false;  // (lane masks: the band test costs two compares and scalar logic)
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const float v = fabsf(acc[r]);
        bool in = v < lo, below = v < hi;
        if (TAIL) {
            const bool ok = row0 + (r & 3) + 8 * (r >> 2) < M;
            in = in && ok;
            below = below && ok;
        }
        cnt += in ? 1 : 0;
        amb = amb | (below ^ in);  // (in implies below: lo <= hi)
    }
    if (__ballot(amb)) {  // rare: the residuals the bf16 product cannot decide, exactly, by their lanes
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float v = fabsf(acc[r]);
            const int i = row0 + (r & 3) + 8 * (r >> 2);
            if (v < hi && !(v < lo) && h_ok && i < M) cnt += exact_inlier(a, p, h, i) ? 1 : 0;
        }
    }
    return cnt;
}

__global__ __launch_bounds__(kMThreads) void support_count_mfma_kernel(SupportArgs a) {
    // a stage: 256 rows of 4 16-B pieces; piece q of row r sits at r * 4 + (q ^ ((r >> 2) & 3)),
    // so that the 16 rows a ds_read_b128 group takes fall on 16 distinct 4-dword bank slots
    __shared__ uint4 stage[kMStage * 4];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int iters = a.iters;
    const int h = blockIdx.x * kMBlockIters + wave * kMWaveIters + (lane & 31);
    const bool h_ok = h < iters;
    if (!pair_runs(a, p)) {  // a pair that does not run: a row of zeros (block-uniform)
        if (lane < 32 && h_ok) a.counts[(size_t)p * iters + h] = 0;
        return;
    }
    const int M = min(a.mcount[p], a.max_nq), half = lane >> 5;
    const float lo = a.thr_lo, hi = a.thr_hi;
    // the wave's B fragments: element j of fragment c is k = 16 c + 8 half + j of iteration h
    // (h < ipad: the image is padded to the block's 128 iterations)
    const uint4* bsrc = (const uint4*)a.eimg + ((size_t)p * a.ipad + h) * 4;
    const uint4 b0 = bsrc[half], b1 = bsrc[2 + half];
    bf16x8 bf0, bf1;
    memcpy(&bf0, &b0, 16);
    memcpy(&bf1, &b1, 16);
    const int flagged = a.xflag[(size_t)p * a.ipad + h];
    const uint4* asrc = (const uint4*)a.uimg + (size_t)p * a.mpad * 4;  // (mpad: multiple of 256)
    int cnt = 0;
    uint4 pre[4];
#pragma unroll
    for (int j = 0; j < 4; j++) pre[j] = M > 0 ? asrc[tid + kMThreads * j] : make_uint4(0, 0, 0, 0);
    for (int m0 = 0; m0 < M; m0 += kMStage) {
        __syncthreads();  // (the previous stage's reads are done)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int g = tid + kMThreads * j, r = g >> 2, q = g & 3;
            stage[r * 4 + (q ^ ((r >> 2) & 3))] = pre[j];
        }
        __syncthreads();
        if (m0 + kMStage < M) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                pre[j] = asrc[(size_t)(m0 + kMStage) * 4 + tid + kMThreads * j];
        }
        const int ntiles = min(kMStage, M - m0 + kMTile - 1) / kMTile;  // (block-uniform)
        for (int t = 0; t < ntiles; t++) {
            const int r = t * kMTile + (lane & 31), sw = (r >> 2) & 3;
            const uint4 a0 = stage[r * 4 + (half ^ sw)], a1 = stage[r * 4 + ((2 + half) ^ sw)];
            bf16x8 af0, af1;
            memcpy(&af0, &a0, 16);
            memcpy(&af1, &a1, 16);
            f32x16 acc;
#pragma unroll
            for (int k = 0; k < 16; k++) acc[k] = 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af0, bf0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af1, bf1, acc, 0, 0, 0);
            const int row0 = m0 + t * kMTile + 4 * half;
            if (m0 + (t + 1) * kMTile <= M)  // (block-uniform)
                cnt += support_epilogue<false>(a, acc, p, h, h_ok, row0, M, lo, hi);
            else
                cnt += support_epilogue<true>(a, acc, p, h, h_ok, row0, M, lo, hi);
        }
    }
    cnt += __shfl_xor(cnt, 32, 64);
    if (lane >= 32 || !h_ok) return;
    if (flagged) {  // outside the bound's assumptions (file header): the plain fp64 count
        cnt = 0;
        for (int i = 0; i < M; i++) cnt += exact_inlier(a, p, h, i) ? 1 : 0;
    }
    a.counts[(size_t)p * iters + h] = cnt;
}

// ---------------------------------------------------------------------------- select ----
// the consensus' distance between two Euler vectors (src/eight_point.cpp:138-139), in float
__device__ __forceinline__ float support_rdist(const float* x, const float* y) {
    const float dx = x[0] - y[0];
    const float dy = x[1] - y[1];
    const float dz = x[2] - y[2];
    return __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
}

// iteration h's validity marks: bit 0 R1, bit 1 R2 (the records' flags / hl's NaN marks)
__device__ __forceinline__ int support_marks(const SupportArgs& a, int p, int h) {
    if (a.hyps) {
        const erp_hypothesis* hy = a.hyps + (size_t)p * a.iters + h;
        return (hy->R1_valid != 0 ? 1 : 0) | (hy->R2_valid != 0 ? 2 : 0);
    }
    const float* hl = a.hl + (size_t)p * 9 * a.iters + h;
    return (__builtin_isnan(hl[0]) ? 0 : 1) | (__builtin_isnan(hl[(size_t)3 * a.iters]) ? 0 : 2);
}

// iteration h's stored R1 / R2 (which) and T as the estimate wrote them
__device__ __forceinline__ void support_stored(const SupportArgs& a, int p, int h, int which,
                                               float* R, float* T) {
    if (a.hyps) {
        const erp_hypothesis* hy = a.hyps + (size_t)p * a.iters + h;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            R[k] = which ? hy->R2[k] : hy->R1[k];
            T[k] = hy->T[k];
        }
        return;
    }
    const float* hl = a.hl + (size_t)p * 9 * a.iters + h;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        R[k] = hl[(size_t)(3 * which + k) * a.iters];
        T[k] = hl[(size_t)(6 + k) * a.iters];
    }
}

// the pair's records when it does not run (or fails its check): the status and zeros, the
// result record copied as it is
__device__ void support_none(const SupportArgs& a, int p, int32_t status) {
    if (threadIdx.x != 0) return;
    a.support[p] = stage_record<erp_support>(status);
    if (a.winners) a.winners[p] = stage_record<erp_winner>(status);
    if (a.out_results) copy_result(a.out_results + p, a.results + p, [](uint64_t*) {});
}

__global__ __launch_bounds__(kSelThreads) void support_select_kernel(SupportArgs a) {
    __shared__ int wsum[kSelWaves], win[2];
    __shared__ int best_c[kSelWaves], best_h[kSelWaves], nsc[kSelWaves], rows[kSelWaves];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const erp_pair_result* res = a.results + p;
    const int32_t gate = stage_gate(res->status, 0, ERP_OK);
    if (gate != ERP_OK) {  // (block-uniform, as every early return below)
        support_none(a, p, gate);
        return;
    }
    const int iters = a.iters, M = a.mcount[p];
    const int s = (int)(M * a.sample_frac);
    if (M < 1 || M > a.max_nq || s < 1) {  // not what an ERP_OK pair of this run looks like
        support_none(a, p, ERP_INTERNAL);
        return;
    }
    const int32_t* cnt = a.counts + (size_t)p * iters;

    // ---- the first argmax over the scored iterations, and how many are scored ----
    int bc = -1, bh = iters, n = 0;
    for (int h = tid; h < iters; h += kSelThreads) {
        if (!support_marks(a, p, h)) continue;
        n++;
        const int c = cnt[h];
        if (c > bc) {  // (h ascends: the first of the thread's ties stays)
            bc = c;
            bh = h;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o, 64), oh = __shfl_xor(bh, o, 64);
        if (oc > bc || (oc == bc && oh < bh)) {
            bc = oc;
            bh = oh;
        }
        n += __shfl_xor(n, o, 64);
    }
    if (lane == 0) {
        best_c[wave] = bc;
        best_h[wave] = bh;
        nsc[wave] = n;
    }
    __syncthreads();
    bc = best_c[0], bh = best_h[0], n = nsc[0];
#pragma unroll
    for (int w = 1; w < kSelWaves; w++) {
        if (best_c[w] > bc || (best_c[w] == bc && best_h[w] < bh)) {
            bc = best_c[w];
            bh = best_h[w];
        }
        n += nsc[w];
    }
    if (bc < 0 || bh >= iters) {  // an ERP_OK pair has K >= 1 valid rotations
        support_none(a, p, ERP_INTERNAL);
        return;
    }
    const int iter = bh;

    // ---- the rows pushed before it (R1 then R2 per iteration, src/eight_point.cpp:113-126) ----
    int before = 0;
    for (int h = tid; h < iter; h += kSelThreads) before += __popc(support_marks(a, p, h));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) rows[wave] = before;
    __syncthreads();
    before = 0;
#pragma unroll
    for (int w = 0; w < kSelWaves; w++) before += rows[w];

    // ---- the consensus iteration: the one that pushed row min_idx (erp_winner.hpp's locate) ----
    const int min_idx = res->min_idx;
    if (a.hyps) {
        winner_from_records(a.hyps + (size_t)p * iters, iters, min_idx, wsum, win);
    } else {
        if (tid == 0) win[0] = -1;
        __syncthreads();
        int base = 0;
        for (int h0 = 0; h0 < iters; h0 += kSelThreads) {
            const int h = h0 + tid;
            const int mk = h < iters ? support_marks(a, p, h) : 0;
            const int c = __popc(mk);
            int total;
            const int first = base + block_exclusive_scan<kSelThreads>(c, wsum, &total);
            if (c && min_idx >= first && min_idx < first + c) {
                win[0] = h;
                win[1] = ((mk & 1) && min_idx == first) ? 0 : 1;
            }
            base += total;
            __syncthreads();
            if (win[0] >= 0 || base > min_idx) break;
        }
    }
    const int cons = win[0];
    if (cons < 0 || cons >= iters) {  // min_idx names no row
        support_none(a, p, ERP_INTERNAL);
        return;
    }
    if (tid != 0) return;

    // ---- which, the self-check and the records (one lane) ----
    const int mk = support_marks(a, p, iter);
    float R1[3], R2[3], T[3];
    support_stored(a, p, iter, 0, R1, T);
    support_stored(a, p, iter, 1, R2, T);
    int which;
    if (mk == 3)  // the rotation nearer to the consensus' answer; R1 on a tie (the polish's rule)
        which = support_rdist(R1, res->R) <= support_rdist(R2, res->R) ? 0 : 1;
    else
        which = mk == 1 ? 0 : 1;
    const float* R = which ? R2 : R1;
    double e[9];
    solved_e(a, p, iter, s, e);
    Hyp hy;
    estimate_from_e(e, a.valid_abs, hy);
    const float* Rc = which ? hy.R2 : hy.R1;
    bool same = ((hy.R1_valid != 0 ? 1 : 0) | (hy.R2_valid != 0 ? 2 : 0)) == mk;
#pragma unroll
    for (int k = 0; k < 3; k++)
        same = same && __float_as_uint(Rc[k]) == __float_as_uint(R[k]) &&
               __float_as_uint(hy.T[k]) == __float_as_uint(T[k]);
    if (!same) {
        a.support[p] = stage_record<erp_support>(ERP_INTERNAL);
        if (a.winners) a.winners[p] = stage_record<erp_winner>(ERP_INTERNAL);
        if (a.out_results) copy_result(a.out_results + p, res, [](uint64_t*) {});
        return;
    }
    const int row = before + ((which && (mk & 1)) ? 1 : 0);
    erp_support o = stage_record<erp_support>(ERP_OK);
    o.iter = iter;
    o.which = which;
    o.inliers = bc;
    o.scored = n;
    o.consensus_iter = cons;
    o.consensus_inliers = cnt[cons];
    o.row = row;
    a.support[p] = o;
    if (a.winners) {
        erp_winner w = stage_record<erp_winner>(ERP_OK);
        w.iter = iter;
        w.which = which;
        w.sample_n = s;
#pragma unroll
        for (int k = 0; k < 9; k++) w.E[k] = e[k];
        a.winners[p] = w;
    }
    if (a.out_results) {
        static_assert(offsetof(erp_pair_result, min_idx) == 36, "min_idx: the high half of word 4");
        copy_result(a.out_results + p, res, [&](uint64_t* w) {
            auto pack = [](float lo32, float hi32) {
                return (uint64_t)__float_as_uint(lo32) | ((uint64_t)__float_as_uint(hi32) << 32);
            };
            w[0] = pack(R[0], R[1]);
            w[1] = pack(R[2], T[0]);
            w[2] = pack(T[1], T[2]);
            w[4] = (w[4] & 0xffffffffull) | ((uint64_t)(uint32_t)row << 32);
        });
    }
}

}  // namespace

SupportScratch support_scratch(const BatchShape& sh) {
    const size_t P = sh.n_pairs, I = sh.iters;
    SupportScratch s;
    s.ipad = (sh.iters + kMBlockIters - 1) / kMBlockIters * kMBlockIters;
    s.mpad = (sh.max_nq + kMStage - 1) / kMStage * kMStage;
    if (s.mpad == 0) s.mpad = kMStage;
    s.ec64_bytes = P * I * 9 * 8;
    s.eimg_bytes = P * (size_t)s.ipad * 64;   // f32 [16] or bf16 [32] per iteration
    s.xflag_bytes = P * (size_t)s.ipad * 4;
    s.uimg_bytes = P * (size_t)s.mpad * 64;   // f32 SoA [9] (36 B) or bf16 [32] per match
    s.counts_bytes = P * I * 4;
    return s;
}

hipError_t launch_support(const SupportArgs& a, int n_pairs, hipStream_t st) {
    const dim3 gp((a.ipad + 63) / 64, n_pairs);
    ERP_LAUNCH(support_prep_kernel<false>, gp, dim3(64), 0, st, a);
    if (!a.hyps) ERP_LAUNCH(support_prep_kernel<true>, gp, dim3(64), 0, st, a);
    ERP_LAUNCH(support_points_kernel, dim3(a.mpad / 256, n_pairs), dim3(256), 0, st, a);
    if (a.mfma)
        ERP_LAUNCH(support_count_mfma_kernel, dim3(a.ipad / kMBlockIters, n_pairs),
                   dim3(kMThreads), 0, st, a);
    else
        ERP_LAUNCH(support_count_valu_kernel, dim3((a.iters + 63) / 64, n_pairs), dim3(64), 0,
                   st, a);
    ERP_LAUNCH(support_select_kernel, dim3((unsigned)n_pairs), dim3(kSelThreads), 0, st, a);
    return hipGetLastError();
}

void support_band(double thr, bool mfma, float* lo, float* hi) {
    const double d = mfma ? kMBand : (double)kVBand;
    float l = thr > d ? (float)(thr - d) : 0.0f, h = (float)(thr + d);
    if (mfma) {  // the f32 below / above: the constants' own rounding only widens the band
        if (l > 0.0f && (double)l >= thr - d) l = __builtin_nextafterf(l, 0.0f);
        if ((double)h <= thr + d) h = __builtin_nextafterf(h, __builtin_huge_valf());
    }
    *lo = l;
    *hi = h;
}

}  // namespace erp

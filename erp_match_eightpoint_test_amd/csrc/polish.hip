// polish.hip -- the polish stage (include/erp_match.h "polish"; no reference counterpart): the
// inlier set of find's winner and an iterated refit on it, for a batch of pairs.  It reads what
// erp_pair_batch_run / erp_eight_point_find_dev wrote (result records, hypothesis records,
// gathered keypoints) and draws no rand().
//
// One workgroup of 256 threads per pair runs every round inside one launch:
//   winner    block prefix scan over the records' two validity flags -> the iteration and the
//             rotation (R1 / R2) that pushed row min_idx (erp_winner.hpp).  The strided read of
//             the 120-B records is the stage's only large traffic (<= n_pairs x iters x 120 B;
//             it stops at the 256-record chunk that holds the winner).  erp_polish_winners_dev
//             takes both and the start E from the pair's erp_winner record instead: no records.
//   pass      every match's residual under E' (9 doubles broadcast through LDS): a wave takes 64
//             consecutive matches per step, its ballot is one 64-bit word of the LDS bitmap
//             (M <= 65535: 8 KB, two of them -- the accepted set and the candidate), the wave's
//             popcount the count.  The same pass adds the inliers' 36 Gram products into
//             per-thread fp64 sums, reduced in a fixed order (lane butterfly, then the four waves
//             one after the other): the next round's refit needs no pass of its own.
//   solve     lane 0: gram_min_eigvec9 (what gram_select_vec runs from 9 rows on; a refit never
//             has fewer), estimate_from_e, the nearest-rotation and T-sign rules, rank2_correct.
// Bearings (pixel_to_bearing: two fp64 sincos per keypoint) are recomputed in every pass: keeping
// them in a context scratch slot (n_pairs x key_stride x 48 B) measured the same time (DESIGN.md
// 3.15), so the stage allocates nothing.  No atomics, no floating-point value depends on another
// pair or on timing: the outputs of a pair are bit-identical from run to run and whatever else is
// in the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/erp_match.h"
#include "erp_ctx.hpp"
#include "erp_device.hpp"
#include "erp_launch.hpp"
#include "erp_stage.hpp"
#include "erp_winner.hpp"

using erp::CtxCall;

namespace {

using namespace erp;

constexpr int kPolishThreads = kWinnerThreads;  // (winner_from_records' block)
constexpr int kPolishWaves = kPolishThreads / 64;
constexpr int kPolishWords = (kStageMaxM + 63) / 64;   // 64-bit words of one bitmap
constexpr int kPolishMinFit = 9;   // below it the thin-SVD rule applies (erp_match.h)

struct PolishArgs {
    erp_polish_inputs in;
    double valid_abs;
    double thr;
    int32_t rounds;
    erp_polish_result* out;
    erp_polish_round* rounds_out;   // may be null
    uint8_t* mask;                  // may be null
    const erp_winner* winners;      // null: the winner comes from in.hyps (erp_polish_dev)
};

// a state of the chain: the solved e, its rank-2 corrected E', the chosen rotation and T
struct PolishState {
    double e[9];
    double Ec[9];
    float R[3];
    float T[3];
    int32_t which;
    int32_t ok;
};

// the consensus' distance between two Euler vectors (src/eight_point.cpp:138-139), in float
__device__ __forceinline__ float polish_rdist(const float* a, const float* b) {
    const float dx = a[0] - b[0];
    const float dy = a[1] - b[1];
    const float dz = a[2] - b[2];
    return __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
}

// One pass over the pair's matches under E' = Ec: the set into bm_new (words [0, ceil(M / 64))),
// the inliers' Gram sums into g36_out, the count as return value; *differs = the set is not
// bm_old's.  Ends with every thread past a barrier (the LDS results are visible).
__device__ int polish_pass(const double* Ec_lds, double thr, int M, const erp_point2f* kl,
                           const erp_point2f* kr, int W, int H, uint64_t* bm_new,
                           const uint64_t* bm_old, double* g36_out, double (*red)[kPolishWaves],
                           int* wcnt, int* wdiff, int* differs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double Ec[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Ec[k] = Ec_lds[k];
    double g[36];
#pragma unroll
    for (int k = 0; k < 36; k++) g[k] = 0.0;
    int cnt = 0, diff = 0;
    for (int c0 = wave * 64; c0 < M; c0 += kPolishThreads) {  // wave-uniform bounds
        const int i = c0 + lane;
        bool in = false;
        double l[3] = {0, 0, 0}, r[3] = {0, 0, 0};
        if (i < M) {
            pixel_to_bearing(W, H, kl[i].x, kl[i].y, l);
            pixel_to_bearing(W, H, kr[i].x, kr[i].y, r);
            in = fabs(inlier_residual(Ec, l, r)) < thr;
        }
        const uint64_t word = __ballot(in);
        cnt += __popcll(word);
        diff |= word != bm_old[c0 >> 6];
        if (lane == 0) bm_new[c0 >> 6] = word;
        if (in) {
            const double LL[6] = {l[0] * l[0], l[0] * l[1], l[0] * l[2],
                                  l[1] * l[1], l[1] * l[2], l[2] * l[2]};
            const double RR[6] = {r[0] * r[0], r[0] * r[1], r[0] * r[2],
                                  r[1] * r[1], r[1] * r[2], r[2] * r[2]};
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int b = 0; b < 6; b++)
                    g[6 * a + b] = __builtin_fma(LL[a], RR[b], g[6 * a + b]);
        }
    }
    // fixed-order reduction: the lane butterfly of each wave, then wave 0 + 1 + 2 + 3
#pragma unroll
    for (int k = 0; k < 36; k++) {
        double v = g[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[k][wave] = v;
    }
    if (lane == 0) {
        wcnt[wave] = cnt;
        wdiff[wave] = diff;
    }
    __syncthreads();
    if (tid < 36) g36_out[tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    int total = 0, d = 0;
#pragma unroll
    for (int w = 0; w < kPolishWaves; w++) {
        total += wcnt[w];
        d |= wdiff[w];
    }
    *differs = d;
    __syncthreads();
    return total;
}

// the pair's round records from round `from` on to zero
__device__ void polish_zero_rounds(const PolishArgs& a, int p, int from) {
    if (!a.rounds_out) return;
    stage_zero<kPolishThreads>((int32_t*)(a.rounds_out + (size_t)p * a.rounds + from),
                               (a.rounds - from) * (int64_t)(sizeof(erp_polish_round) / 4));
}

// the pair's outputs when it does not run: the status and zeros
__device__ void polish_skip(const PolishArgs& a, int p, int32_t status) {
    if (threadIdx.x == 0) a.out[p] = stage_record<erp_polish_result>(status);
    polish_zero_rounds(a, p, 0);
    if (a.mask) stage_zero<kPolishThreads>(a.mask + (size_t)p * a.in.key_stride, a.in.key_stride);
}

__global__ __launch_bounds__(kPolishThreads) void polish_kernel(PolishArgs a) {
    __shared__ uint64_t bm[2][kPolishWords];
    __shared__ double g36[2][36];
    __shared__ double red[36][kPolishWaves];
    __shared__ PolishState acc, prop;
    __shared__ int wsum[kPolishWaves], wcnt[kPolishWaves], wdiff[kPolishWaves];
    __shared__ int win[2];

    const int p = blockIdx.x, tid = threadIdx.x;
    const erp_pair_result* res = a.in.results + p;
    const int64_t stride = a.in.key_stride;
    const int64_t m64 = stage_match_count(res, stride);
    const erp_winner* wr = a.winners ? a.winners + p : nullptr;  // (erp_polish_winners_dev)
    const int32_t gate = stage_gate(res->status, m64, wr ? wr->status : (int32_t)ERP_OK);
    if (gate != ERP_OK) {  // (block-uniform)
        polish_skip(a, p, gate);
        return;
    }
    const int M = (int)m64;

    // ---- the winner: the record whose R1 / R2 was pushed as row min_idx, from the records'
    // flags (erp_winner.hpp) or, for erp_polish_winners_dev, from the pair's winner record ----
    const double* e0;
    if (wr) {  // (block-uniform)
        if (tid == 0) {
            win[0] = wr->iter;
            win[1] = wr->which;
        }
        __syncthreads();
        e0 = wr->E;
    } else {
        const erp_hypothesis* hyps = a.in.hyps + (size_t)p * a.in.iters;
        winner_from_records(hyps, a.in.iters, res->min_idx, wsum, win);
        if (win[0] < 0) {  // min_idx names no row of these records
            polish_skip(a, p, ERP_INTERNAL);
            return;
        }
        e0 = hyps[win[0]].E;
    }
    const int winner = win[0], winner_which = win[1];

    // ---- the start state: the winner's E, the result record's R and T ----
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) acc.e[k] = e0[k];
        rank2_correct(acc.e, acc.Ec);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            acc.R[k] = res->R[k];
            acc.T[k] = res->T[k];
        }
        acc.which = winner_which;
    }
    __syncthreads();

    const erp_point2f* kl = a.in.key_left + (size_t)p * stride;
    const erp_point2f* kr = a.in.key_right + (size_t)p * stride;
    const int W = a.in.width[p], H = a.in.height[p];
    int cur = 0, differs = 0;
    // (bm[1] is compared against before it holds a set: the flag of this pass is not used)
    for (int k = tid; k < (M + 63) / 64; k += kPolishThreads) bm[1][k] = 0;
    __syncthreads();
    int n_cur = polish_pass(acc.Ec, a.thr, M, kl, kr, W, H, bm[0], bm[1], g36[0], red, wcnt, wdiff,
                            &differs);
    const int n_winner = n_cur;
    int done = 0;
    for (int r = 1; r <= a.rounds; r++) {
        if (n_cur < kPolishMinFit) break;
        if (tid == 0) {
            double g[36];
#pragma unroll
            for (int k = 0; k < 36; k++) g[k] = g36[cur][k];
            gram_min_eigvec9(g, 1, 0, prop.e);
            Hyp hy;
            estimate_from_e(prop.e, a.valid_abs, hy);
            prop.ok = hy.R1_valid || hy.R2_valid;
            if (prop.ok) {
                // the candidate nearer to the previous rotation; R1 on a tie
                const bool first = hy.R1_valid &&
                                   (!hy.R2_valid || polish_rdist(hy.R1, acc.R) <= polish_rdist(hy.R2, acc.R));
                prop.which = first ? 0 : 1;
                double dot = (double)hy.T[0] * (double)acc.T[0];
                dot = dot + (double)hy.T[1] * (double)acc.T[1];
                dot = dot + (double)hy.T[2] * (double)acc.T[2];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    prop.R[k] = first ? hy.R1[k] : hy.R2[k];
                    prop.T[k] = dot < 0 ? -hy.T[k] : hy.T[k];
                }
                rank2_correct(prop.e, prop.Ec);
            }
        }
        __syncthreads();
        if (!prop.ok) break;
        const int n_new = polish_pass(prop.Ec, a.thr, M, kl, kr, W, H, bm[cur ^ 1], bm[cur],
                                      g36[cur ^ 1], red, wcnt, wdiff, &differs);
        if (n_new < n_cur) break;  // the round is discarded
        if (tid == 0) {
            acc = prop;
            if (a.rounds_out) {
                erp_polish_round o;
                memset(&o, 0, sizeof(o));
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    o.R[k] = prop.R[k];
                    o.T[k] = prop.T[k];
                }
                o.n_fit = n_cur;
                o.n_inliers = n_new;
                o.which = prop.which;
#pragma unroll
                for (int k = 0; k < 9; k++) o.E[k] = prop.e[k];
                a.rounds_out[(size_t)p * a.rounds + (r - 1)] = o;
            }
        }
        __syncthreads();
        cur ^= 1;
        n_cur = n_new;
        done = r;
        if (!differs) break;  // the fixed point: further rounds would repeat this one
    }

    // ---- outputs ----
    if (tid == 0) {
        erp_polish_result o = stage_record<erp_polish_result>(ERP_OK);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o.R[k] = acc.R[k];
            o.T[k] = acc.T[k];
        }
        o.winner_iter = winner;
        o.winner_which = winner_which;
        o.rounds_done = done;
        o.n_inliers = n_cur;
        o.n_inliers_winner = n_winner;
#pragma unroll
        for (int k = 0; k < 9; k++) o.E[k] = acc.e[k];
        a.out[p] = o;
    }
    polish_zero_rounds(a, p, done);
    if (a.mask) {
        uint8_t* m = a.mask + (size_t)p * stride;
        for (int64_t i = tid; i < stride; i += kPolishThreads)
            m[i] = i < M ? (uint8_t)((bm[cur][i >> 6] >> (i & 63)) & 1) : (uint8_t)0;
    }
}

}  // namespace

extern "C" {

// erp_polish_dev (winners == nullptr: the winner from in->hyps) and erp_polish_winners_dev
static erp_status polish_call(erp_ctx* ctx, const erp_polish_inputs* in, const erp_winner* winners,
                              bool from_winners, double valid_abs, float thr, int32_t rounds,
                              erp_polish_result* d_out, erp_polish_round* d_rounds,
                              uint8_t* d_mask, void* stream) {
    if (!ctx || !in || !(thr > 0) || rounds < 0 || rounds > kPolishMaxRounds || in->n_pairs < 0 ||
        (!from_winners && in->iters < 1) || in->key_stride < 0)
        return ERP_INVALID_ARG;
    if (in->n_pairs == 0) return ERP_OK;
    if (!d_out || !in->results || !(from_winners ? (const void*)winners : (const void*)in->hyps) ||
        !in->width || !in->height || (in->key_stride > 0 && (!in->key_left || !in->key_right)))
        return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    PolishArgs a{};
    a.in = *in;
    a.valid_abs = valid_abs;
    a.thr = (double)thr;
    a.rounds = rounds;
    a.out = d_out;
    a.rounds_out = rounds > 0 ? d_rounds : nullptr;
    a.mask = d_mask;
    a.winners = from_winners ? winners : nullptr;
    ERP_LAUNCH_S(polish_kernel, dim3((unsigned)in->n_pairs), dim3(kPolishThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? ERP_OK : ERP_HIP_ERROR;
}

erp_status erp_polish_dev(erp_ctx* ctx, const erp_polish_inputs* in, double valid_abs, float thr,
                          int32_t rounds, erp_polish_result* d_out, erp_polish_round* d_rounds,
                          uint8_t* d_mask, void* stream) {
    return polish_call(ctx, in, nullptr, false, valid_abs, thr, rounds, d_out, d_rounds, d_mask,
                       stream);
}

erp_status erp_polish_winners_dev(erp_ctx* ctx, const erp_polish_inputs* in,
                                  const erp_winner* d_winners, double valid_abs, float thr,
                                  int32_t rounds, erp_polish_result* d_out,
                                  erp_polish_round* d_rounds, uint8_t* d_mask, void* stream) {
    return polish_call(ctx, in, d_winners, true, valid_abs, thr, rounds, d_out, d_rounds, d_mask,
                       stream);
}

erp_status erp_eight_point_find_polished(erp_ctx* ctx, int32_t W, int32_t H,
                                         const erp_point2f* h_kl, const erp_point2f* h_kr,
                                         int32_t m, const erp_ransac_cfg* cfg, float thr,
                                         int32_t rounds, erp_pair_result* h_result,
                                         erp_polish_result* h_polish, uint8_t* h_mask) {
    // (the polish's arguments first: a call that fails on them must not consume a rand stream)
    if (!ctx || !cfg || cfg->iters < 1 || m < 0 || m > kStageMaxM || (m > 0 && (!h_kl || !h_kr)) ||
        !(thr > 0) || rounds < 0 || rounds > kPolishMaxRounds)
        return ERP_INVALID_ARG;
    // one lock across upload, find, polish and download: the staging buffers are the context's
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    const PolishedStage L(m, cfg->iters);
    erp_status s = upload_keys(ctx, h_kl, h_kr, m);
    if (s != ERP_OK) return s;
    char* base = ctx_scratch<char>(ctx, kSlotHostStage, L.bytes);
    if (!base || !ensure(ctx->in_c, sizeof(erp_pair_result))) return ERP_OUT_OF_MEMORY;
    erp_hypothesis* d_hyps = (erp_hypothesis*)(base + L.hyps);
    erp_polish_result* d_pol = (erp_polish_result*)(base + L.polish);
    int32_t* d_wh = (int32_t*)(base + L.wh);
    uint8_t* d_mask = (uint8_t*)(base + L.mask);
    erp_pair_result* d_res = (erp_pair_result*)ctx->in_c.p;
    const int32_t wh[2] = {W, H};
    ERP_CK(hipMemcpy(d_wh, wh, sizeof(wh), hipMemcpyHostToDevice));
    s = erp_eight_point_find_dev(ctx, W, H, keys_left(ctx), keys_right(ctx), m, cfg, d_res, d_hyps,
                                 nullptr);
    if (s != ERP_OK) return s;
    erp_polish_inputs in = one_pair_inputs<erp_polish_inputs>(ctx, m, d_wh, d_res);
    in.iters = cfg->iters;
    in.hyps = d_hyps;
    s = erp_polish_dev(ctx, &in, cfg->valid_abs, thr, rounds, d_pol, nullptr, d_mask, nullptr);
    if (s != ERP_OK) return s;
    erp_pair_result r;
    ERP_CK(hipMemcpy(&r, d_res, sizeof(r), hipMemcpyDeviceToHost));
    if (h_result) *h_result = r;
    if (h_polish) ERP_CK(hipMemcpy(h_polish, d_pol, sizeof(*h_polish), hipMemcpyDeviceToHost));
    if (h_mask && m > 0) ERP_CK(hipMemcpy(h_mask, d_mask, (size_t)m, hipMemcpyDeviceToHost));
    return (erp_status)r.status;
}

}  // extern "C"

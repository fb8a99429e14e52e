// pose.hip -- the pose selection (include/erp_match.h "pose selection"; no reference
// counterpart): the cheirality vote over (R1 | R2) x (+t | -t) for a batch of pairs, with the
// depths of the matches under the selected pose.  It reads what find, the winner records and
// the polish wrote (result records, a solved 9-vector per pair, gathered keypoints, optionally
// an inlier mask) and changes none of it; it draws no rand().
//
// One workgroup of 256 threads per pair, one launch:
//   candidates  lane 0: rank2_correct and decompose_e (erp_device.hpp, what find runs); E', R1,
//               R2 and t go to the other lanes through LDS (30 doubles).
//   pass 1      a wave takes 64 consecutive matches per step: bearings, the optional residual
//               test, the depths under R1 and R2 (under -t both change sign exactly, so once per
//               rotation).  The four vote predicates and the voter predicate are ballots; their
//               popcounts go into per-wave integer counts, summed wave 0 + 1 + 2 + 3 from LDS.
//   selection   every thread from the five totals (block-uniform): most votes, lowest k on a tie.
//   pass 2      only when depth or front is asked for: the selected rotation's depths again (the
//               same function on the same inputs: the same bits) -> depth, front, zeros from M
//               up to key_stride.
// Bearings are recomputed in each pass as the polish does (DESIGN.md 3.15 measured a scratch copy
// at the same time).  No atomics, no floating-point sum across matches at all: the outputs of a
// pair are bit-identical from run to run and whatever else is in the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include <cmath>
#include <mutex>

#include "../../include/erp_match.h"
#include "erp_ctx.hpp"
#include "erp_device.hpp"
#include "erp_launch.hpp"
#include "erp_stage.hpp"

using erp::CtxCall;

namespace {

using namespace erp;

constexpr int kPoseThreads = 256;
constexpr int kPoseWaves = kPoseThreads / 64;

struct PoseArgs {
    erp_pose_inputs in;
    double thr;        // <= 0: no residual test
    double min_sin2;
    erp_pose* out;
    double* depth;               // may be null
    uint8_t* front;              // may be null
    erp_pair_result* results_out;  // may be null
};

// what lane 0 leaves in LDS for the block
struct PoseCand {
    double Ec[9];
    double R[2][9];
    double t[3];
};

// rule 2 for one rotation: the depths along l and r under (Rc, +t) and the squared sine of the
// parallax; products and sums left to right as the header writes them
__device__ __forceinline__ void pose_depths(const double* Rc, const double* t, const double* l,
                                            const double* r, double* d_l, double* d_r,
                                            double* det_out) {
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = Rc[3 * i] * r[0] + Rc[3 * i + 1] * r[1] + Rc[3 * i + 2] * r[2];
    const double a = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
    const double b = l[0] * q[0] + l[1] * q[1] + l[2] * q[2];
    const double c = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
    const double lt = l[0] * t[0] + l[1] * t[1] + l[2] * t[2];
    const double qt = q[0] * t[0] + q[1] * t[1] + q[2] * t[2];
    const double det = a * c - b * b;
    *d_l = (c * lt - b * qt) / det;
    *d_r = (b * lt - a * qt) / det;
    *det_out = det;
}

// match i's bearings and whether it passes the mask and threshold tests (rule 3, first two)
__device__ __forceinline__ bool pose_match(const PoseArgs& a, const PoseCand& cd, int i, int W,
                                           int H, const erp_point2f* kl, const erp_point2f* kr,
                                           const uint8_t* mask, double* l, double* r) {
    pixel_to_bearing(W, H, kl[i].x, kl[i].y, l);
    pixel_to_bearing(W, H, kr[i].x, kr[i].y, r);
    bool ok = !mask || mask[i] != 0;
    if (a.thr > 0) ok = ok && fabs(inlier_residual(cd.Ec, l, r)) < a.thr;
    return ok;
}

// the pair's result record into results_out, R and T replaced when given
__device__ __forceinline__ void pose_copy_result(const PoseArgs& a, int p, const float* R,
                                                 const float* T) {
    if (!a.results_out || threadIdx.x != 0) return;
    copy_result(a.results_out + p, a.in.results + p, [=](uint64_t* w) {
        if (!R) return;
        const uint32_t f[6] = {__float_as_uint(R[0]), __float_as_uint(R[1]), __float_as_uint(R[2]),
                               __float_as_uint(T[0]), __float_as_uint(T[1]), __float_as_uint(T[2])};
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = (uint64_t)f[2 * k] | ((uint64_t)f[2 * k + 1] << 32);
    });
}

// depth and front of slots [from, key_stride) to zero
__device__ __forceinline__ void pose_zero_tail(const PoseArgs& a, int p, int64_t from) {
    const int64_t stride = a.in.key_stride;
    if (a.depth)
        stage_zero<kPoseThreads>(a.depth + ((size_t)p * stride + from) * 2, 2 * (stride - from));
    if (a.front) stage_zero<kPoseThreads>(a.front + (size_t)p * stride + from, stride - from);
}

// the pair's outputs when no pose is selected: the status and zeros, the result record as it is
__device__ __forceinline__ void pose_skip(const PoseArgs& a, int p, int32_t status, const int* votes,
                          int n_voters) {
    if (threadIdx.x == 0) {
        erp_pose o = stage_record<erp_pose>(status);
        if (votes) {
#pragma unroll
            for (int k = 0; k < 4; k++) o.votes[k] = votes[k];
            o.n_voters = n_voters;
        }
        a.out[p] = o;
    }
    pose_zero_tail(a, p, 0);
    pose_copy_result(a, p, nullptr, nullptr);
}

__global__ __launch_bounds__(kPoseThreads) void pose_kernel(PoseArgs a) {
    __shared__ PoseCand cd;
    __shared__ int wcnt[5][kPoseWaves];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const erp_pair_result* res = a.in.results + p;
    const int64_t stride = a.in.key_stride;
    const int64_t m64 = stage_match_count(res, stride);
    const RecordSource src = source_of(a.in);
    const int32_t gate = stage_gate(res->status, m64, src.status_of(p));
    if (gate != ERP_OK) {  // (block-uniform, as every branch on a status)
        pose_skip(a, p, gate, nullptr, 0);
        return;
    }
    const int M = (int)m64;

    // ---- candidates (rule 1) ----
    if (tid == 0) {
        const double* e = src.e_of(p);
        double e9[9];
#pragma unroll
        for (int k = 0; k < 9; k++) e9[k] = e[k];
        rank2_correct(e9, cd.Ec);
        decompose_e(cd.Ec, cd.R[0], cd.R[1], cd.t);
    }
    __syncthreads();

    const erp_point2f* kl = a.in.key_left + (size_t)p * stride;
    const erp_point2f* kr = a.in.key_right + (size_t)p * stride;
    const uint8_t* mask = a.in.mask ? a.in.mask + (size_t)p * stride : nullptr;
    const int W = a.in.width[p], H = a.in.height[p];

    // ---- pass 1: the votes (rules 2 and 3) ----
    int cnt[5] = {0, 0, 0, 0, 0};
    for (int c0 = wave * 64; c0 < M; c0 += kPoseThreads) {  // wave-uniform bounds
        const int i = c0 + lane;
        bool v[4] = {false, false, false, false}, voter = false;
        if (i < M) {
            double l[3], r[3];
            if (pose_match(a, cd, i, W, H, kl, kr, mask, l, r)) {
#pragma unroll
                for (int w = 0; w < 2; w++) {
                    double dl, dr, det;
                    pose_depths(cd.R[w], cd.t, l, r, &dl, &dr, &det);
                    const bool par = det > 0 && det >= a.min_sin2;
                    v[2 * w] = par && dl > 0 && dr > 0;
                    v[2 * w + 1] = par && dl < 0 && dr < 0;
                    voter = voter || par;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) cnt[k] += __popcll(__ballot(v[k]));
        cnt[4] += __popcll(__ballot(voter));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; k++) wcnt[k][wave] = cnt[k];
    }
    __syncthreads();
    int tot[5];
#pragma unroll
    for (int k = 0; k < 5; k++) tot[k] = ((wcnt[k][0] + wcnt[k][1]) + wcnt[k][2]) + wcnt[k][3];

    // ---- selection (rule 4) ----
    if (tot[4] == 0) {
        pose_skip(a, p, ERP_TOO_FEW_POINTS, tot, 0);
        return;
    }
    int best = 0, most = tot[0];
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (tot[k] > most) {
            most = tot[k];
            best = k;
        }
    const int which = best >> 1, neg = best & 1;
    const double sg = neg ? -1.0 : 1.0;

    // ---- the record (rule 5) ----
    if (tid == 0) {
        erp_pose o = stage_record<erp_pose>(ERP_OK);
        o.which = which;
        o.t_sign = neg ? -1 : 1;
        o.n_voters = tot[4];
#pragma unroll
        for (int k = 0; k < 4; k++) o.votes[k] = tot[k];
        double eu[3];
        rot2eular(cd.R[which], eu);
        bool same = true;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            o.R[k] = (float)eu[k];
            o.t[k] = sg * cd.t[k];
            o.T[k] = (float)o.t[k];
            // (byte for byte: the bit patterns, so -0 differs from 0 and a NaN equals itself)
            same = same && __float_as_uint(o.R[k]) == __float_as_uint(res->R[k]);
        }
#pragma unroll
        for (int k = 0; k < 9; k++) o.Rm[k] = cd.R[which][k];
        double dot = (double)o.T[0] * (double)res->T[0];
        dot = dot + (double)o.T[1] * (double)res->T[1];
        dot = dot + (double)o.T[2] * (double)res->T[2];
        o.rot_agrees = same ? 1 : 0;
        o.t_flipped = dot < 0 ? 1 : 0;
        a.out[p] = o;
        pose_copy_result(a, p, o.R, o.T);
    }
    if (!a.depth && !a.front) return;  // (block-uniform)

    // ---- pass 2: the selected pose's depths and votes (rule 6) ----
    double* dout = a.depth ? a.depth + (size_t)p * stride * 2 : nullptr;
    uint8_t* fout = a.front ? a.front + (size_t)p * stride : nullptr;
    for (int i = tid; i < M; i += kPoseThreads) {
        double l[3], r[3], dl = 0.0, dr = 0.0;
        bool fr = false;
        if (pose_match(a, cd, i, W, H, kl, kr, mask, l, r)) {
            double xl, xr, det;
            pose_depths(cd.R[which], cd.t, l, r, &xl, &xr, &det);
            if (det > 0 && det >= a.min_sin2) {
                dl = sg * xl;
                dr = sg * xr;
                fr = dl > 0 && dr > 0;
            }
        }
        if (dout) {
            dout[2 * (size_t)i] = dl;
            dout[2 * (size_t)i + 1] = dr;
        }
        if (fout) fout[i] = fr ? 1 : 0;
    }
    pose_zero_tail(a, p, M);
}

}  // namespace

extern "C" {

erp_status erp_pose_select_dev(erp_ctx* ctx, const erp_pose_inputs* in, float thr, double min_sin2,
                               erp_pose* d_out, double* d_depth, uint8_t* d_front,
                               erp_pair_result* d_results_out, void* stream) {
    if (!ctx || !in || !(min_sin2 >= 0) || std::isnan(thr) || in->n_pairs < 0 ||
        in->key_stride < 0)
        return ERP_INVALID_ARG;
    if (in->n_pairs == 0) return ERP_OK;
    if (!d_out || !in->results || !in->width || !in->height ||
        (in->key_stride > 0 && (!in->key_left || !in->key_right)) || !source_ok(source_of(*in)))
        return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    PoseArgs a{};
    a.in = *in;
    a.thr = (double)thr;
    a.min_sin2 = min_sin2;
    a.out = d_out;
    a.depth = d_depth;
    a.front = d_front;
    a.results_out = d_results_out;
    ERP_LAUNCH_S(pose_kernel, dim3((unsigned)in->n_pairs), dim3(kPoseThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? ERP_OK : ERP_HIP_ERROR;
}

erp_status erp_eight_point_find_posed(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* h_kl,
                                      const erp_point2f* h_kr, int32_t m,
                                      const erp_ransac_cfg* cfg, float thr, int32_t rounds,
                                      double min_sin2, erp_pair_result* h_result,
                                      erp_polish_result* h_polish, erp_pose* h_pose,
                                      uint8_t* h_mask, double* h_depth, uint8_t* h_front) {
    // (the later stages' arguments first: a call that fails on them must not consume a rand stream)
    if (!ctx || !cfg || cfg->iters < 1 || m < 0 || m > kStageMaxM || (m > 0 && (!h_kl || !h_kr)) ||
        !(thr > 0) || rounds < 0 || rounds > kPolishMaxRounds || !(min_sin2 >= 0))
        return ERP_INVALID_ARG;
    // one lock across upload, find, polish, selection and download: the staging buffers are the
    // context's
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    const PosedStage L(m);
    erp_status s = upload_keys(ctx, h_kl, h_kr, m);
    if (s != ERP_OK) return s;
    char* base = ctx_scratch<char>(ctx, kSlotHostStage, L.bytes);
    if (!base) return ERP_OUT_OF_MEMORY;
    erp_pair_result* d_res = (erp_pair_result*)(base + L.result);
    erp_winner* d_win = (erp_winner*)(base + L.winner);
    erp_polish_result* d_pol = (erp_polish_result*)(base + L.polish);
    erp_pose* d_pose = (erp_pose*)(base + L.pose);
    int32_t* d_wh = (int32_t*)(base + L.wh);
    double* d_depth = (double*)(base + L.depth);
    uint8_t* d_mask = (uint8_t*)(base + L.mask);
    uint8_t* d_front = (uint8_t*)(base + L.front);
    const int32_t wh[2] = {W, H};
    ERP_CK(hipMemcpy(d_wh, wh, sizeof(wh), hipMemcpyHostToDevice));
    s = erp_eight_point_find_winner_dev(ctx, W, H, keys_left(ctx), keys_right(ctx), m, cfg, d_res,
                                        nullptr, d_win, nullptr);
    if (s != ERP_OK) return s;
    const erp_polish_inputs pin = one_pair_inputs<erp_polish_inputs>(ctx, m, d_wh, d_res);
    s = erp_polish_winners_dev(ctx, &pin, d_win, cfg->valid_abs, thr, rounds, d_pol, nullptr,
                               d_mask, nullptr);
    if (s != ERP_OK) return s;
    erp_pose_inputs in = one_pair_inputs<erp_pose_inputs>(ctx, m, d_wh, d_res);
    in.e = d_pol->E;
    in.e_stride = sizeof(erp_polish_result);
    in.src_status = &d_pol->status;
    in.src_status_stride = sizeof(erp_polish_result);
    in.mask = d_mask;
    s = erp_pose_select_dev(ctx, &in, 0.0f, min_sin2, d_pose, h_depth ? d_depth : nullptr,
                            h_front ? d_front : nullptr, nullptr, nullptr);
    if (s != ERP_OK) return s;
    erp_pair_result r;
    ERP_CK(hipMemcpy(&r, d_res, sizeof(r), hipMemcpyDeviceToHost));
    if (h_result) *h_result = r;
    if (h_polish) ERP_CK(hipMemcpy(h_polish, d_pol, sizeof(*h_polish), hipMemcpyDeviceToHost));
    if (h_pose) ERP_CK(hipMemcpy(h_pose, d_pose, sizeof(*h_pose), hipMemcpyDeviceToHost));
    if (m > 0) {
        if (h_mask) ERP_CK(hipMemcpy(h_mask, d_mask, (size_t)m, hipMemcpyDeviceToHost));
        if (h_depth) ERP_CK(hipMemcpy(h_depth, d_depth, (size_t)m * 16, hipMemcpyDeviceToHost));
        if (h_front) ERP_CK(hipMemcpy(h_front, d_front, (size_t)m, hipMemcpyDeviceToHost));
    }
    return (erp_status)r.status;
}

}  // extern "C"

// sweep.hip -- rotation sweeps (include/erp_match.h, "rotation sweep"): what the reference's
// three experiment drivers run per pose, for a list of poses and without leaving the device.
//
//   one_image_test/main.cpp:73-145            5^3 poses, left = right base, + the match error
//   two_synthesis_image_test/main.cpp:80-141  16^3 poses
//   two_real_image_test/main.cpp:169-230      16^3 poses
//     im2 = rotate_image(im_right, rot_mat.inv())      rotate_images_enqueue (remap_api.hip)
//     do_all(im_left, im2, ...)                         the left image's bands + SURF ONCE per
//                                                       call, the right ones group by group,
//                                                       pack_enqueue with a shared left side
//     degree_error mean (one_image_test :27-50,         match_error_kernel (here)
//       :115-129)
//     eight_point::find                                 erp_pair_batch_run
//
// The left image's features do not depend on the pose, so its four bands go through the remap
// and SURF once and every pair's left rows are copies of them; only one group's rotated right
// images exist at a time.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/erp_match.h"
#include "erp_ctx.hpp"
#include "erp_device.hpp"
#include "erp_image_batch.hpp"
#include "erp_launch.hpp"
#include "erp_remap.hpp"
#include "erp_surf.hpp"

namespace {

using erp::ctx_scratch;
using erp::CtxCall;

// ---- the match error (one_image_test/main.cpp:27-50, :115-129) ----
constexpr int kMePairsPerLaunch = 32;  // poses per launch: their matrices travel as kernel
constexpr int kMeThreads = 256;        // arguments (32 x 72 B), so nothing outlives the call

struct MatchErrorArgs {
    double m[kMePairsPerLaunch][9];  // rot_mat of pairs pair0 .. (row-major)
    const erp_point2f* key_left;
    const erp_point2f* key_right;
    const int32_t* m_count;
    double* out;
    int64_t key_stride, m_stride;
    int32_t pair0, W, H;
};

// degree_error(vec1, vec2, width, height) :27-50, every step in the written order
__device__ __forceinline__ double degree_error(erp_point2f v1, erp_point2f v2, int32_t W,
                                               int32_t H) {
    const double a1 = erp::kPi * (double)v1.y / (double)H;
    const double b1 = 2 * erp::kPi * (double)v1.x / (double)W;
    const double a2 = erp::kPi * (double)v2.y / (double)H;
    const double b2 = 2 * erp::kPi * (double)v2.x / (double)W;
    const double x1 = sin(a1) * cos(b1), y1 = sin(a1) * sin(b1), z1 = cos(a1);
    const double x2 = sin(a2) * cos(b2), y2 = sin(a2) * sin(b2), z2 = cos(a2);
    const double product = x1 * x2 + y1 * y2 + z1 * z2;
    double error_rad = 0;
    if (product < 1) error_rad = acos(product);
    return error_rad;
}

// One workgroup per pair.  Per chunk of 256 matches every lane computes one term into LDS,
// then lane 0 adds the chunk's terms to the running sum in match order (std::accumulate's
// order, whatever the launch shape); the mean is sum / M, NaN for M = 0 as in the reference.
__global__ __launch_bounds__(kMeThreads) void match_error_kernel(const MatchErrorArgs a) {
    __shared__ double term[kMeThreads];
    const int tid = threadIdx.x;
    const size_t p = (size_t)a.pair0 + blockIdx.x;
    // a negative count is no match; a count past the pair's slots reads only its own slots
    const int32_t M =
        (int32_t)min((int64_t)max(a.m_count[p * (size_t)a.m_stride], 0), a.key_stride);
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = a.m[blockIdx.x][k];
    const erp_point2f* __restrict__ kl = a.key_left + p * (size_t)a.key_stride;
    const erp_point2f* __restrict__ kr = a.key_right + p * (size_t)a.key_stride;
    double sum = 0.0;
    for (int32_t i0 = 0; i0 < M; i0 += kMeThreads) {
        const int32_t i = i0 + tid;
        if (i < M) {
            const erp_point2f l = kl[i];
            // Vec2i(left_key.pt.y, left_key.pt.x) -> rotate_pixel(., rot_mat) -> Point2f(col, row)
            int32_t r, c;
            erp::rotate_pixel(erp::trunc_i32_x86f(l.y), erp::trunc_i32_x86f(l.x), m, a.W, a.H, &r,
                              &c);
            erp_point2f v1;
            v1.x = (float)c;
            v1.y = (float)r;
            term[tid] = degree_error(v1, kr[i], a.W, a.H);
        }
        __syncthreads();
        if (tid == 0) {
            const int32_t n = min(M - i0, kMeThreads);
            for (int32_t k = 0; k < n; k++) sum = sum + term[k];
        }
        __syncthreads();
    }
    if (tid == 0) a.out[p] = sum / (double)M;
}

bool match_error_args_ok(const erp_point2f* kl, const erp_point2f* kr, int64_t key_stride,
                         const int32_t* d_m, int64_t m_stride, int32_t n_pairs,
                         const double* h_rot_mat, int32_t W, int32_t H, const double* d_out) {
    return n_pairs >= 0 && n_pairs <= (1 << 24) && key_stride >= 0 && m_stride >= 1 && W > 0 &&
           H > 0 && (n_pairs == 0 || (kl && kr && d_m && h_rot_mat && d_out));
}

// the launches of erp_match_error_dev (the caller holds the context's call section)
erp_status match_error_enqueue(const erp_point2f* kl, const erp_point2f* kr, int64_t key_stride,
                               const int32_t* d_m, int64_t m_stride, int32_t n_pairs,
                               const double* h_rot_mat, int32_t W, int32_t H, double* d_out,
                               hipStream_t st) {
    for (int32_t p0 = 0; p0 < n_pairs; p0 += kMePairsPerLaunch) {
        const int32_t n = std::min(kMePairsPerLaunch, n_pairs - p0);
        MatchErrorArgs a{};
        for (int32_t k = 0; k < n; k++)
            for (int q = 0; q < 9; q++) a.m[k][q] = h_rot_mat[(size_t)(p0 + k) * 9 + q];
        a.key_left = kl;
        a.key_right = kr;
        a.m_count = d_m;
        a.out = d_out;
        a.key_stride = key_stride;
        a.m_stride = m_stride;
        a.pair0 = p0;
        a.W = W;
        a.H = H;
        ERP_LAUNCH_S(match_error_kernel, dim3((unsigned)n), dim3(kMeThreads), 0, st, a);
    }
    return hipGetLastError() == hipSuccess ? ERP_OK : ERP_HIP_ERROR;
}

// ---- the features stage ----
// the matrices rotate_pixel applies for the poses: rot_mat_inv = rot_mat.inv() is what the
// drivers hand to rotate_image, which inverts its argument again (src/erp_rotation.cpp:103)
bool pose_matrices(const double* h_rot_mat, int32_t n_poses, std::vector<double>* m) {
    m->resize((size_t)n_poses * 9);
    for (int32_t p = 0; p < n_poses; p++) {
        double inv[9];
        if (!erp_inv3(h_rot_mat + (size_t)p * 9, inv) || !erp_inv3(inv, m->data() + (size_t)p * 9))
            return false;
    }
    return true;
}

erp_status sweep_features_checked(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_base,
                                  int32_t n_poses, const double* h_rot_mat, int32_t W, int32_t H,
                                  const erp_surf_params* prm, int32_t max_kp, int32_t fill,
                                  int32_t max_group_pairs, const erp_packed_pairs* out,
                                  erp_image_batch_info* info, hipStream_t st) {
    if (!ctx || !info) return ERP_INVALID_ARG;
    *info = erp_image_batch_info{};
    if (n_poses < 0 || n_poses > (1 << 24) || !erp::image_dims_ok(W, H) ||
        !erp::surf_args_ok(W, H / 4, 3, prm, max_kp) || fill < 0 || fill > 255 ||
        max_group_pairs < 0 || !erp::packed_ok(out) ||
        (n_poses > 0 && (!d_left || !d_base || !h_rot_mat)))
        return ERP_INVALID_ARG;
    std::vector<double> mats;
    if (!pose_matrices(h_rot_mat, n_poses, &mats)) return ERP_INVALID_ARG;  // before any GPU work
    if (hipSetDevice(ctx->device) != hipSuccess) return ERP_HIP_ERROR;
    CtxCall call(ctx, st);
    if (n_poses == 0) {
        if (hipMemsetAsync(out->off_l, 0, sizeof(int64_t), st) != hipSuccess ||
            hipMemsetAsync(out->off_r, 0, sizeof(int64_t), st) != hipSuccess)
            return ERP_HIP_ERROR;
        info->fits = 1;
        return ERP_OK;
    }
    const int32_t Hb = H / 4;
    const size_t img = (size_t)W * H * 3, band = (size_t)Hb * W * 3;
    const size_t K = (size_t)max_kp;
    // One band image's share of the budget (SURF scratch, its canvas, its padded output); a
    // pair adds four of them and one rotated image; the left image's four are there whatever
    // the group (its SURF scratch is the group's, used before the first group).
    const size_t per_band = erp::surf_scratch_bytes_per_image(W, Hb, 3, prm, max_kp) + band +
                            K * (sizeof(erp_keypoint) + 64 * 4) + sizeof(int32_t);
    const size_t per_pair = 4 * per_band + img;
    const size_t fixed = 4 * (K * (sizeof(erp_keypoint) + 64 * 4) + sizeof(int32_t));
    const size_t budget = erp::kGroupBudgetBytes > fixed ? erp::kGroupBudgetBytes - fixed : 0;
    int32_t g = max_group_pairs > 0
                    ? max_group_pairs
                    : (int32_t)std::min<size_t>(std::max<size_t>(budget / per_pair, 1),
                                                (size_t)erp::kMaxAutoGroupPairs);
    g = std::min(g, n_poses);
    // the band canvases hold the left image's four bands first, then each group's 4 g
    uint8_t* bands = ctx_scratch<uint8_t>(ctx, erp::kSlotBands, (size_t)g * 4 * band);
    uint8_t* canvas = ctx_scratch<uint8_t>(ctx, erp::kSlotSweepCanvas, (size_t)g * img);
    erp_keypoint* kp =
        ctx_scratch<erp_keypoint>(ctx, erp::kSlotKp, (size_t)g * 4 * K * sizeof(erp_keypoint));
    float* desc = ctx_scratch<float>(ctx, erp::kSlotDesc, (size_t)g * 4 * K * 64 * 4);
    int32_t* cnt = ctx_scratch<int32_t>(ctx, erp::kSlotCount, (size_t)g * 4 * sizeof(int32_t));
    erp_keypoint* lkp =
        ctx_scratch<erp_keypoint>(ctx, erp::kSlotLeftKp, 4 * K * sizeof(erp_keypoint));
    float* ldesc = ctx_scratch<float>(ctx, erp::kSlotLeftDesc, 4 * K * 64 * 4);
    int32_t* lcnt = ctx_scratch<int32_t>(ctx, erp::kSlotLeftCount, 4 * sizeof(int32_t));
    if (!bands || !canvas || !kp || !desc || !cnt || !lkp || !ldesc || !lcnt)
        return ERP_OUT_OF_MEMORY;
    int32_t raw_max = 0;
    // the left image: bands + SURF once per call
    if (hipMemsetAsync(bands, fill, 4 * band, st) != hipSuccess) return ERP_HIP_ERROR;
    erp_status s = erp::spherical_bands_enqueue(ctx, d_left, 1, W, H, bands, 4 * band, st);
    if (s == ERP_OK)
        s = erp::surf_detect_compute_enqueue(ctx, bands, 4, W, Hb, 3, prm, max_kp, lkp, ldesc, lcnt,
                                             st, &raw_max);
    if (s != ERP_OK) return s;
    for (int32_t p0 = 0; p0 < n_poses; p0 += g) {
        const int32_t gp = std::min(g, n_poses - p0);
        if (hipMemsetAsync(canvas, fill, (size_t)gp * img, st) != hipSuccess ||
            hipMemsetAsync(bands, fill, (size_t)gp * 4 * band, st) != hipSuccess)
            return ERP_HIP_ERROR;
        s = erp::rotate_images_enqueue(ctx, d_base, gp, mats.data() + (size_t)p0 * 9, W, H, canvas,
                                       st);
        if (s == ERP_OK)
            s = erp::spherical_bands_enqueue(ctx, canvas, gp, W, H, bands, 4 * band, st);
        if (s == ERP_OK)
            s = erp::surf_detect_compute_enqueue(ctx, bands, gp * 4, W, Hb, 3, prm, max_kp, kp,
                                                 desc, cnt, st, &raw_max);
        if (s == ERP_OK) {
            // every pair's left bands are the left image's; its right bands this group's
            const erp::PackSide side[2] = {{lkp, ldesc, lcnt, 0, 0}, {kp, desc, cnt, 4, 0}};
            s = erp::pack_enqueue(ctx, side, gp, max_kp, p0, W, H, *out, st);
        }
        if (s != ERP_OK) return s;
        info->groups++;
    }
    return erp::packed_totals(*out, n_poses, max_kp, raw_max, info, st);
}

}  // namespace

extern "C" {

erp_status erp_match_error_dev(erp_ctx* ctx, const erp_point2f* d_key_left,
                               const erp_point2f* d_key_right, int64_t key_stride,
                               const int32_t* d_m, int64_t m_stride, int32_t n_pairs,
                               const double* h_rot_mat, int32_t W, int32_t H, double* d_out,
                               void* stream) {
    if (!ctx || !match_error_args_ok(d_key_left, d_key_right, key_stride, d_m, m_stride, n_pairs,
                                     h_rot_mat, W, H, d_out))
        return ERP_INVALID_ARG;
    if (n_pairs == 0) return ERP_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return ERP_HIP_ERROR;
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    return match_error_enqueue(d_key_left, d_key_right, key_stride, d_m, m_stride, n_pairs,
                               h_rot_mat, W, H, d_out, st);
}

erp_status erp_image_sweep_features_dev(erp_ctx* ctx, const uint8_t* d_left,
                                        const uint8_t* d_right_base, int32_t n_poses,
                                        const double* h_rot_mat, int32_t W, int32_t H,
                                        const erp_surf_params* params, int32_t max_kp,
                                        int32_t fill, int32_t max_group_pairs,
                                        const erp_packed_pairs* out, erp_image_batch_info* info,
                                        void* stream) {
    return sweep_features_checked(ctx, d_left, d_right_base, n_poses, h_rot_mat, W, H, params,
                                  max_kp, fill, max_group_pairs, out, info, (hipStream_t)stream);
}

erp_status erp_image_sweep_run(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right_base,
                               int32_t n_poses, const double* h_rot_mat, int32_t W, int32_t H,
                               const erp_surf_params* params, int32_t max_kp, int32_t fill,
                               int32_t max_group_pairs, const erp_packed_pairs* packed,
                               float ratio, const erp_ransac_cfg* cfg,
                               const erp_batch_outputs* out, double* d_match_error,
                               erp_image_batch_info* info, void* stream) {
    if (!cfg || !out || !out->results) return ERP_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    // each stage leaves the context's call section before the next takes it
    erp_status s = sweep_features_checked(ctx, d_left, d_right_base, n_poses, h_rot_mat, W, H,
                                          params, max_kp, fill, max_group_pairs, packed, info, st);
    if (s != ERP_OK || !info->fits || n_poses == 0) return s;
    erp_batch_outputs o = *out;
    if (d_match_error) {
        // the matched keypoints the match error reads: the caller's where given, else scratch
        const size_t kb = (size_t)n_poses * (size_t)std::max(info->max_nq, 1) * sizeof(erp_point2f);
        if (!o.key_left)
            o.key_left = ctx_scratch<erp_point2f>(ctx, erp::kSlotSweepKeyL, kb);
        if (!o.key_right)
            o.key_right = ctx_scratch<erp_point2f>(ctx, erp::kSlotSweepKeyR, kb);
        if (!o.key_left || !o.key_right) return ERP_OUT_OF_MEMORY;
    }
    s = erp::packed_batch_run(ctx, *packed, n_poses, *info, ratio, cfg, &o, st);
    if (s != ERP_OK || !d_match_error) return s;
    CtxCall call(ctx, st);
    return match_error_enqueue(o.key_left, o.key_right, info->max_nq, &out->results[0].M,
                               (int64_t)(sizeof(erp_pair_result) / sizeof(int32_t)), n_poses,
                               h_rot_mat, W, H, d_match_error, st);
}

}  // extern "C"

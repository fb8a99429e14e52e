// image_batch.hip -- batched do_all (include/erp_match.h, "batched do_all"): ERP image pairs ->
// the packed pair batch erp_pair_batch_run consumes, without leaving the device.
//
//   spherical_surf::do_all   src/spherical_surf.cpp:65-179
//     bands                  :77-93    erp::spherical_bands_enqueue (remap_api.hip)
//     SURF on the 8 bands    :96-118   erp::surf_detect_compute_enqueue (surf_api.hip)
//     un-rotation + concat   :120-150  pack_offsets_kernel + pack_rows_kernel (here)
//
// The pack step turns SURF's padded per-band output ([8 P][max_kp] slots, counts on the device)
// into the ragged concatenation n0, n1, n2, n3 per side and pair.  Two launches cover a whole
// call whatever the pair count: pack_offsets_kernel scans the counts into the pair offsets and
// the first output row of every band; pack_rows_kernel moves the rows.  The descriptor move is
// a pure copy of 256-byte rows (16 lanes x 16 B per row, HBM bound); the keypoints go through
// the same device function as band_keypoints_kernel (erp_remap.hpp unrotate_band_keypoint).
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

constexpr int kPackRowsPerBlock = 16;  // 256 threads = 16 rows x 16 lanes of 16 B
constexpr int kPackMaxBlocksPerBand = 16;

struct PackArgs {
    double m[4][9];      // per band: rotate_keypoint's matrix (band 1 unused: the shift band)
    erp_packed_pairs o;
    erp::PackSide s[2];  // where each side's band images are (left, right)
    int64_t* row_base;   // [8 n_pairs] first output row of every band (scratch)
    int32_t n_pairs, max_kp, pair0, W, H;
};

__device__ __forceinline__ int32_t clamp_count(int32_t c, int32_t max_kp) {
    return min(max(c, 0), max_kp);
}
// the band image holding band `band` of pair p's side
__device__ __forceinline__ size_t src_image(const erp::PackSide& s, int p, int band) {
    return (size_t)s.first + (size_t)p * s.pair_stride + band;
}

// One block: the group's pair offsets (appended after out.off_*[pair0], which the previous
// group's launch wrote; pair0 == 0 starts at row 0), width / height / band_counts, and the
// first output row of each of the 8 n_pairs bands.  256 pairs per step, inclusive scan in LDS.
__global__ __launch_bounds__(256) void pack_offsets_kernel(PackArgs a) {
    __shared__ int64_t sl[256], sr[256];
    __shared__ int64_t carry[2];
    const int tid = threadIdx.x;
    if (tid == 0) {
        carry[0] = a.pair0 ? a.o.off_l[a.pair0] : 0;
        carry[1] = a.pair0 ? a.o.off_r[a.pair0] : 0;
        if (a.pair0 == 0) {
            a.o.off_l[0] = 0;
            a.o.off_r[0] = 0;
        }
    }
    __syncthreads();
    for (int p0 = 0; p0 < a.n_pairs; p0 += 256) {
        const int p = p0 + tid;
        int32_t c[8];
        int64_t nl = 0, nr = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            c[k] = p < a.n_pairs
                       ? clamp_count(a.s[k >> 2].count[src_image(a.s[k >> 2], p, k & 3)], a.max_kp)
                       : 0;
            if (k < 4) nl += c[k];
            else nr += c[k];
        }
        sl[tid] = nl;
        sr[tid] = nr;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t vl = tid >= d ? sl[tid - d] : 0, vr = tid >= d ? sr[tid - d] : 0;
            __syncthreads();
            sl[tid] += vl;
            sr[tid] += vr;
            __syncthreads();
        }
        const int64_t base_l = carry[0], base_r = carry[1];
        if (p < a.n_pairs) {
            const size_t g = (size_t)a.pair0 + p;
            int64_t rl = base_l + sl[tid] - nl, rr = base_r + sr[tid] - nr;
            a.o.off_l[g + 1] = base_l + sl[tid];
            a.o.off_r[g + 1] = base_r + sr[tid];
            a.o.width[g] = a.W;
            a.o.height[g] = a.H;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (a.o.band_counts) a.o.band_counts[g * 8 + k] = c[k];
                if (k < 4) {
                    a.row_base[(size_t)p * 8 + k] = rl;
                    rl += c[k];
                } else {
                    a.row_base[(size_t)p * 8 + k] = rr;
                    rr += c[k];
                }
            }
        }
        __syncthreads();
        if (tid == 255) {
            carry[0] = base_l + sl[255];
            carry[1] = base_r + sr[255];
        }
        __syncthreads();
    }
}

// blockIdx.x = output band ([pair][side][band]; its rows come from the band image the side's
// PackSide maps it to), blockIdx.y strides over its rows.  Rows at or
// past the band's count are not read; rows at or past the side's capacity are not written.
__global__ __launch_bounds__(256) void pack_rows_kernel(PackArgs a) {
    const int side = (int)(blockIdx.x >> 2) & 1, band = (int)blockIdx.x & 3;
    const erp::PackSide& s = a.s[side];
    const size_t img = src_image(s, (int)(blockIdx.x >> 3), band);
    const int32_t n = clamp_count(s.count[img], a.max_kp);
    if (n == 0) return;
    const int64_t base = a.row_base[blockIdx.x];
    const int64_t cap = side ? a.o.cap_r : a.o.cap_l;
    const int tid = threadIdx.x;
    // descriptors: consecutive lanes on consecutive 16-byte pieces of a 256-byte row
    const float4* __restrict__ src = (const float4*)s.desc + img * (size_t)a.max_kp * 16;
    float4* __restrict__ dst = (float4*)(side ? a.o.desc_r : a.o.desc_l);
    const int lane = tid & 15;
    for (int r = blockIdx.y * kPackRowsPerBlock + (tid >> 4); r < n;
         r += gridDim.y * kPackRowsPerBlock) {
        const int64_t row = base + r;
        if (row >= cap) break;
        dst[(size_t)row * 16 + lane] = src[(size_t)r * 16 + lane];
    }
    // keypoints: pt of the cv::KeyPoint records -> un-rotated ERP pixels
    const erp_keypoint* __restrict__ ksrc = s.kp + img * (size_t)a.max_kp;
    erp_point2f* __restrict__ kdst = side ? a.o.kp_r : a.o.kp_l;
    for (int r = blockIdx.y * 256 + tid; r < n; r += gridDim.y * 256) {
        const int64_t row = base + r;
        if (row >= cap) break;
        erp_point2f p;
        p.x = ksrc[r].x;
        p.y = ksrc[r].y;
        kdst[row] = erp::unrotate_band_keypoint(p, band == 1, a.m[band], a.W, a.H);
    }
}

}  // namespace

namespace erp {

bool image_dims_ok(int32_t W, int32_t H) {
    return W > 0 && H >= 4 && (int64_t)W * H <= ((int64_t)1 << 31) / 3;
}

bool packed_ok(const erp_packed_pairs* o) {
    return o && o->desc_l && o->desc_r && o->kp_l && o->kp_r && o->off_l && o->off_r &&
           o->width && o->height && o->cap_l >= 0 && o->cap_r >= 0 &&
           ((uintptr_t)o->desc_l & 15) == 0 && ((uintptr_t)o->desc_r & 15) == 0;
}

erp_status pack_enqueue(erp_ctx* ctx, const PackSide side[2], int32_t n_pairs, int32_t max_kp,
                        int32_t pair0, int32_t W, int32_t H, const erp_packed_pairs& out,
                        hipStream_t st) {
    static const float pitch[4] = {45.f, 0.f, -45.f, -90.f};  // do_all :121-126
    PackArgs a{};
    for (int b = 0; b < 4; b++)
        if (b != 1) erp::pitch_matrix(pitch[b], a.m[b]);
    a.o = out;
    a.s[0] = side[0];
    a.s[1] = side[1];
    a.row_base = ctx_scratch<int64_t>(ctx, kSlotRowBase, (size_t)n_pairs * 8 * sizeof(int64_t));
    if (!a.row_base) return ERP_OUT_OF_MEMORY;
    a.n_pairs = n_pairs;
    a.max_kp = max_kp;
    a.pair0 = pair0;
    a.W = W;
    a.H = H;
    ERP_LAUNCH_S(pack_offsets_kernel, dim3(1), dim3(256), 0, st, a);
    const int by = std::min(kPackMaxBlocksPerBand,
                            (max_kp + kPackRowsPerBlock - 1) / kPackRowsPerBlock);
    ERP_LAUNCH_S(pack_rows_kernel, dim3((unsigned)n_pairs * 8, by), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? ERP_OK : ERP_HIP_ERROR;
}

erp_status packed_totals(const erp_packed_pairs& out, int32_t n_pairs, int32_t max_kp,
                         int32_t raw_max, erp_image_batch_info* info, hipStream_t st) {
    std::vector<int64_t> off(2 * ((size_t)n_pairs + 1));
    const size_t ob = ((size_t)n_pairs + 1) * sizeof(int64_t);
    if (hipMemcpyAsync(off.data(), out.off_l, ob, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(off.data() + n_pairs + 1, out.off_r, ob, hipMemcpyDeviceToHost, st) !=
            hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return ERP_HIP_ERROR;
    const int64_t* ol = off.data();
    const int64_t* orr = off.data() + n_pairs + 1;
    int64_t mq = 0, mt = 0;
    for (int32_t p = 0; p < n_pairs; p++) {
        mq = std::max(mq, ol[p + 1] - ol[p]);
        mt = std::max(mt, orr[p + 1] - orr[p]);
    }
    info->need_kp = raw_max;
    info->max_nq = (int32_t)mq;  // <= 4 max_kp
    info->max_nt = (int32_t)mt;
    info->rows_l = ol[n_pairs];
    info->rows_r = orr[n_pairs];
    info->fits = raw_max <= max_kp && info->rows_l <= out.cap_l && info->rows_r <= out.cap_r;
    return ERP_OK;
}

erp_status packed_batch_run(erp_ctx* ctx, const erp_packed_pairs& packed, int32_t n_pairs,
                            const erp_image_batch_info& info, float ratio,
                            const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                            hipStream_t st) {
    erp_pair_batch b{};
    b.n_pairs = n_pairs;
    b.dim = 64;
    b.max_nq = info.max_nq;
    b.max_nt = info.max_nt;
    b.desc_l = packed.desc_l;
    b.desc_r = packed.desc_r;
    b.kp_l = packed.kp_l;
    b.kp_r = packed.kp_r;
    b.off_l = packed.off_l;
    b.off_r = packed.off_r;
    b.width = packed.width;
    b.height = packed.height;
    return erp_pair_batch_run(ctx, &b, ratio, cfg, out, (void*)st);
}

}  // namespace erp

namespace {

using erp::ctx_scratch;
using erp::CtxCall;
using erp::kSlotBands;
using erp::kSlotCount;
using erp::kSlotDesc;
using erp::kSlotKp;

// both sides of pairs whose band images lie [pair][left, right][n0..n3] in one array
erp_status pack_pairs_enqueue(erp_ctx* ctx, const erp_keypoint* d_kp, const float* d_desc,
                              const int32_t* d_count, int32_t n_pairs, int32_t max_kp,
                              int32_t pair0, int32_t W, int32_t H, const erp_packed_pairs& out,
                              hipStream_t st) {
    const erp::PackSide side[2] = {{d_kp, d_desc, d_count, 8, 0}, {d_kp, d_desc, d_count, 8, 4}};
    return erp::pack_enqueue(ctx, side, n_pairs, max_kp, pair0, W, H, out, st);
}

erp_status features_checked(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                            int32_t n_pairs, int32_t W, int32_t H, const erp_surf_params* prm,
                            int32_t max_kp, int32_t fill, int32_t max_group_pairs,
                            const erp_packed_pairs* out, erp_image_batch_info* info,
                            hipStream_t st) {
    if (!ctx || !info) return ERP_INVALID_ARG;
    *info = erp_image_batch_info{};
    if (n_pairs < 0 || n_pairs > (1 << 24) || !erp::image_dims_ok(W, H) ||
        !erp::surf_args_ok(W, H / 4, 3, prm, max_kp) || fill < 0 || fill > 255 ||
        max_group_pairs < 0 || !erp::packed_ok(out) || (n_pairs > 0 && (!d_left || !d_right)))
        return ERP_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ERP_HIP_ERROR;
    CtxCall call(ctx, st);
    if (n_pairs == 0) {
        if (hipMemsetAsync(out->off_l, 0, sizeof(int64_t), st) != hipSuccess ||
            hipMemsetAsync(out->off_r, 0, sizeof(int64_t), st) != hipSuccess)
            return ERP_HIP_ERROR;
        info->fits = 1;
        return ERP_OK;
    }
    const int32_t Hb = H / 4;
    const size_t img = (size_t)W * H * 3, band = (size_t)Hb * W * 3;
    const size_t K = (size_t)max_kp;
    // group size: everything that grows with the pair count, against the budget
    const size_t per_pair = 8 * (erp::surf_scratch_bytes_per_image(W, Hb, 3, prm, max_kp) + band +
                                 K * (sizeof(erp_keypoint) + 64 * 4) + sizeof(int32_t));
    int32_t g = max_group_pairs > 0
                    ? max_group_pairs
                    : (int32_t)std::min<size_t>(
                          std::max<size_t>(erp::kGroupBudgetBytes / per_pair, 1),
                          (size_t)erp::kMaxAutoGroupPairs);
    g = std::min(g, n_pairs);
    uint8_t* bands = ctx_scratch<uint8_t>(ctx, kSlotBands, (size_t)g * 8 * band);
    erp_keypoint* kp =
        ctx_scratch<erp_keypoint>(ctx, kSlotKp, (size_t)g * 8 * K * sizeof(erp_keypoint));
    float* desc = ctx_scratch<float>(ctx, kSlotDesc, (size_t)g * 8 * K * 64 * 4);
    int32_t* cnt = ctx_scratch<int32_t>(ctx, kSlotCount, (size_t)g * 8 * sizeof(int32_t));
    if (!bands || !kp || !desc || !cnt) return ERP_OUT_OF_MEMORY;
    int32_t raw_max = 0;
    for (int32_t p0 = 0; p0 < n_pairs; p0 += g) {
        const int32_t gp = std::min(g, n_pairs - p0);
        if (hipMemsetAsync(bands, fill, (size_t)gp * 8 * band, st) != hipSuccess)
            return ERP_HIP_ERROR;
        // band sets in the order [pair][left, right]: each side's images are strided by a pair
        erp_status s = erp::spherical_bands_enqueue(ctx, d_left + (size_t)p0 * img, gp, W, H, bands,
                                                    8 * band, st);
        if (s == ERP_OK)
            s = erp::spherical_bands_enqueue(ctx, d_right + (size_t)p0 * img, gp, W, H,
                                             bands + 4 * band, 8 * band, st);
        if (s == ERP_OK)
            s = erp::surf_detect_compute_enqueue(ctx, bands, gp * 8, W, Hb, 3, prm, max_kp, kp,
                                                 desc, cnt, st, &raw_max);
        if (s == ERP_OK)
            s = pack_pairs_enqueue(ctx, kp, desc, cnt, gp, max_kp, p0, W, H, *out, st);
        if (s != ERP_OK) return s;
        info->groups++;
    }
    // the totals for the caller: one copy + sync per call
    return erp::packed_totals(*out, n_pairs, max_kp, raw_max, info, st);
}

}  // namespace

extern "C" {

erp_status erp_pack_band_features_dev(erp_ctx* ctx, const erp_keypoint* d_kp, const float* d_desc,
                                      const int32_t* d_count, int32_t n_pairs, int32_t max_kp,
                                      int32_t W, int32_t H, const erp_packed_pairs* out,
                                      void* stream) {
    if (!ctx || n_pairs < 0 || n_pairs > (1 << 24) || max_kp < 1 || !erp::image_dims_ok(W, H) ||
        !erp::packed_ok(out) || (n_pairs > 0 && (!d_kp || !d_desc || !d_count)) ||
        ((uintptr_t)d_desc & 15) != 0)
        return ERP_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ERP_HIP_ERROR;
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    if (n_pairs == 0)
        return hipMemsetAsync(out->off_l, 0, sizeof(int64_t), st) == hipSuccess &&
                       hipMemsetAsync(out->off_r, 0, sizeof(int64_t), st) == hipSuccess
                   ? ERP_OK
                   : ERP_HIP_ERROR;
    return pack_pairs_enqueue(ctx, d_kp, d_desc, d_count, n_pairs, max_kp, 0, W, H, *out, st);
}

erp_status erp_image_pairs_features_dev(erp_ctx* ctx, const uint8_t* d_left,
                                        const uint8_t* d_right, int32_t n_pairs, int32_t W,
                                        int32_t H, const erp_surf_params* params, int32_t max_kp,
                                        int32_t fill, int32_t max_group_pairs,
                                        const erp_packed_pairs* out, erp_image_batch_info* info,
                                        void* stream) {
    return features_checked(ctx, d_left, d_right, n_pairs, W, H, params, max_kp, fill,
                            max_group_pairs, out, info, (hipStream_t)stream);
}

erp_status erp_image_pairs_run(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                               int32_t n_pairs, int32_t W, int32_t H,
                               const erp_surf_params* params, int32_t max_kp, int32_t fill,
                               int32_t max_group_pairs, const erp_packed_pairs* packed,
                               float ratio, const erp_ransac_cfg* cfg,
                               const erp_batch_outputs* out, erp_image_batch_info* info,
                               void* stream) {
    if (!cfg || !out || !out->results) return ERP_INVALID_ARG;
    // the features call leaves the context's call section before the batch call takes it
    const erp_status s = features_checked(ctx, d_left, d_right, n_pairs, W, H, params, max_kp,
                                          fill, max_group_pairs, packed, info,
                                          (hipStream_t)stream);
    if (s != ERP_OK || !info->fits || n_pairs == 0) return s;
    return erp::packed_batch_run(ctx, *packed, n_pairs, *info, ratio, cfg, out,
                                 (hipStream_t)stream);
}

}  // extern "C"


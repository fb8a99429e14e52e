// erp_remap.hpp -- launchers of the ERP pixel-remap kernels (remap.hip): the spherical band
// remap of spherical_surf::do_all and the rectification remaps of automatic.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/erp_match.h"
#ifdef __HIPCC__
#include "erp_device.hpp"
#endif

namespace erp {

enum RemapMode : int32_t {
    kRemapCrop = 0,   // crop_rotated_image: output rows r <- source rows row0 + r, rotated
    kRemapCopy = 1,   // the unrotated band: rows [row0, row0 + rows) copied
    kRemapFull = 2,   // rotate_image: every pixel of the H x W image
    kRemapRot90 = 3   // rotate_image, then cv::rotate(ROTATE_90_CLOCKWISE): W x H output
};

struct RemapJob {
    const uint8_t* src;  // H x W x 3 (BGR bytes, row-major)
    uint8_t* dst;
    double m[9];         // the matrix rotate_pixel applies (row-major)
    int32_t row0;        // source row of output row 0 (crop / copy)
    int32_t rows;        // output rows (crop / copy: H/4, full: H)
    int32_t mode;        // RemapMode
    int32_t pad;
};

constexpr int kMaxRemapJobs = 8;
struct RemapJobs {
    RemapJob j[kMaxRemapJobs];
};

// pixels whose truncated values fall within 1e-8 of an integer are deferred to a fix-up kernel
// (correctly rounded transcendentals, erp_device.hpp rotate_pixel_cr): list of
// (job << 32 | output pixel index), sized for every output pixel of the launch
struct RemapScratch {
    uint32_t* count;        // device counter (zeroed by launch_remap)
    uint64_t* list;         // [n_jobs * out_rows * out_cols]
};

// up to kMaxRemapJobs independent remaps of images sharing W x H: the remap launch + the
// boundary fix-up launch
hipError_t launch_remap(const RemapJobs& jobs, int n_jobs, int max_out_rows, int max_out_cols,
                        int W, int H, const RemapScratch& scr, hipStream_t st);

// ONE remap geometry applied to many images (the vertical view's fixed matrix over a batch):
// the source index of an output pixel is the same for every image, so a thread computes it once
// and copies the pixel for every image (remap_shared_kernel).  job gives the geometry -- mode
// (CROP, FULL or ROT90; not COPY), m, row0, rows -- and the first image: image i of the stack is
// job.src + i * src_stride -> job.dst + i * dst_stride (bytes), i < n.  src2 / dst2: an optional
// second stack of n images with the same strides (the right images of a pair batch; NULL = none).
// Sources and destinations must not overlap.
struct RemapSharedArgs {
    RemapJob job;
    const uint8_t* src2;
    uint8_t* dst2;
    int64_t src_stride, dst_stride;
    int32_t n;       // images per stack
    int32_t chunks;  // set by launch_remap_shared: ceil(n / kRemapSharedChunk)
};

// Images per block of the shared-map kernel.  A launch has one grid z-slice per stack and chunk
// of kRemapSharedChunk images, and every slice computes the index again: 16 bounds that
// recomputation at 1/16 of the per-image kernel's arithmetic per image, while batches beyond
// 16 images still spread over more slices (an image size with few blocks needs them to fill
// the device).
constexpr int kRemapSharedChunk = 16;

// the boundary list of a shared-map launch: output pixel indices, one entry per output pixel
// at most (only the first slice appends; the fix-up copies the pixel for every image)
struct RemapSharedScratch {
    uint32_t* count;        // device counter (zeroed by launch_remap_shared)
    uint32_t* list;         // [out_rows * out_cols]
};

// the shared-map launch + its boundary fix-up launch; hipErrorInvalidValue for mode COPY or a
// negative n, nothing to do for n == 0.  a.chunks is ignored on input.
hipError_t launch_remap_shared(const RemapSharedArgs& a, int W, int H,
                               const RemapSharedScratch& scr, hipStream_t st);

// d_out[i] = h_flags[i] != 0 for i < n (int32), from host flags passed as kernel arguments: no
// host memory is read after the call returns
hipError_t launch_set_flags(int32_t* d_out, const int32_t* h_flags, int n, hipStream_t st);

struct BandKeypointArgs {
    double m[4][9];     // per band: rotate_keypoint's matrix (unused for shift_band)
    int32_t end[4];     // exclusive end index of each band's segment in the concatenated list
    int32_t shift_band; // the unrotated band (pt.y += height*3/8), 1 in do_all; -1 = none
    int32_t W, H;
};
hipError_t launch_band_keypoints(erp_point2f* d_kp, const BandKeypointArgs& a, hipStream_t st);

#ifdef __HIPCC__
// do_all's un-rotation of one band keypoint (src/spherical_surf.cpp:120-133): the unrotated
// band shifts pt.y by height*3/8 (float); the others go through rotate_keypoint with the
// band's pitch matrix m (offset_i = pt.y + height*3/8 in float, truncated; col = (int)pt.x).
// Shared by band_keypoints_kernel (remap.hip) and the batch pack kernel (image_batch.hip).
__device__ __forceinline__ erp_point2f unrotate_band_keypoint(erp_point2f p, bool shift,
                                                              const double* m, int32_t W,
                                                              int32_t H) {
    const float off = (float)(H * 3 / 8);
    if (shift) {
        p.y = p.y + off;
    } else {
        const int32_t oi = trunc_i32_x86f(p.y + off);
        const int32_t ci = trunc_i32_x86f(p.x);
        int32_t r, c;
        rotate_pixel(oi, ci, m, W, H, &r, &c);
        p.x = (float)c;
        p.y = (float)r;
    }
    return p;
}
#endif

// the pitch matrix rotate_keypoint / crop_rotated_image build from a float pitch in degrees
// (remap_api.hip)
void pitch_matrix(float deg, double m[9]);
// erp_spherical_bands_dev's launches without its argument checks and call section (the caller
// holds the context's): image i's four bands go to d_bands + i * band_set_stride bytes
erp_status spherical_bands_enqueue(erp_ctx* ctx, const uint8_t* d_ims, int32_t n_images,
                                   int32_t W, int32_t H, uint8_t* d_bands,
                                   size_t band_set_stride, hipStream_t st);
// rotate_image of ONE image by n matrices (m [n][9]: what rotate_pixel applies, i.e. the
// inverse of rotate_image's argument) into n contiguous H x W x 3 outputs, kMaxRemapJobs FULL
// jobs per launch; no argument checks, the caller holds the context's call section
erp_status rotate_images_enqueue(erp_ctx* ctx, const uint8_t* d_im, int32_t n, const double* m,
                                 int32_t W, int32_t H, uint8_t* d_out, hipStream_t st);

}  // namespace erp

// erp_image_batch.hpp -- what the batched do_all (image_batch.hip) shares with the rotation
// sweep (sweep.hip): the pack step over band features that need not lie pair after pair, the
// argument checks of the packed outputs and the group budget.  (Their context scratch slots are
// in erp_ctx.hpp's table.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/erp_match.h"

namespace erp {

// The group budget (DESIGN.md section 3.8 has the A/B): the largest group whose SURF scratch +
// band canvases + staging stay within it, and no more than kMaxAutoGroupPairs pairs.  9 GiB
// holds 8 pairs of 5376 x 2688 (1.08 GB each), the fastest of 4 / 8 / 16 there; at 1344 x 672,
// where the budget would allow ~58 pairs, groups of 8 ran 64 pairs 1.5x faster than one group
// of 64 (SURF's per-band cost grows with the bands per call), hence the cap.
constexpr size_t kGroupBudgetBytes = (size_t)9 << 30;
constexpr int32_t kMaxAutoGroupPairs = 8;

// One side's band features as erp_surf_detect_compute_dev writes them -- kp [images][max_kp],
// desc [images][max_kp][64], count [images] -- and where pair p's bands n0..n3 are among those
// images: first + p * pair_stride + band.  The batched do_all has both sides in one array
// (pair_stride 8, first 0 / 4); the sweep's left side is one image for every pair
// (pair_stride 0).
struct PackSide {
    const erp_keypoint* kp;
    const float* desc;     // 16-byte aligned
    const int32_t* count;
    int32_t pair_stride;
    int32_t first;
};

bool image_dims_ok(int32_t W, int32_t H);           // W > 0, H >= 4, W H 3 < 2^31
bool packed_ok(const erp_packed_pairs* o);          // pointers, capacities, alignment
// the two pack launches for pairs [pair0, pair0 + n_pairs) of a call (the caller holds the
// context's call section); side[] describes these pairs only
erp_status pack_enqueue(erp_ctx* ctx, const PackSide side[2], int32_t n_pairs, int32_t max_kp,
                        int32_t pair0, int32_t W, int32_t H, const erp_packed_pairs& out,
                        hipStream_t st);
// the end of a features call: the pair offsets on the host (one copy + sync) -> info's max_nq,
// max_nt, rows_l, rows_r and fits (need_kp = raw_max, the largest raw count of any band)
erp_status packed_totals(const erp_packed_pairs& out, int32_t n_pairs, int32_t max_kp,
                         int32_t raw_max, erp_image_batch_info* info, hipStream_t st);
// erp_pair_batch_run on a packed batch that fits (dim 64, info's max_nq / max_nt)
erp_status packed_batch_run(erp_ctx* ctx, const erp_packed_pairs& packed, int32_t n_pairs,
                            const erp_image_batch_info& info, float ratio,
                            const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                            hipStream_t st);

}  // namespace erp

// erp/eight_point.hpp -- C++ mirror of the reference's eight_point class (and random_array's
// role) without OpenCV.  Reference: /root/reference/src/eight_point.hpp:8-59.
//
// The hard-coded constants of initial_guess (80 iterations, 25 % samples, 20-80 % trimmed
// mean, 1.57 rad validity) live in `cfg` with the reference values as defaults; the sampler
// replays the reference's process-global glibc rand() stream (seed 1, `cfg.offset` draws
// consumed before).  All work runs on the GPU through the C ABI (include/erp_match.h).
#pragma once

#include <vector>

#include "../erp_match.h"
#include "rand_stream.hpp"
#include "types.hpp"

namespace erp {

class eight_point {
public:
    explicit eight_point(int device = 0);
    ~eight_point();
    eight_point(const eight_point&) = delete;
    eight_point& operator=(const eight_point&) = delete;

    // src/eight_point.hpp:11-14
    void find(int im_width, int im_height, std::vector<KeyPoint>& key_left,
              std::vector<KeyPoint>& key_right, Vec3f& R_vec_out, Vec3f& T_vec_out, int match_size);
    // find followed by the polish stage (erp_match.h "polish"; no reference counterpart): the
    // winner's inliers under |l^T E' r| < thr and up to `rounds` (0..8) refits on them.
    // R_vec_out / T_vec_out: the last accepted state (rounds = 0: find's answer); inlier_mask
    // (may be nullptr) is resized to match_size, 1 = inlier of that state.  last_result() is
    // find's record, last_polish() the polish record.  Draws from the stream as find does.
    void find_polished(int im_width, int im_height, std::vector<KeyPoint>& key_left,
                       std::vector<KeyPoint>& key_right, Vec3f& R_vec_out, Vec3f& T_vec_out,
                       int match_size, float thr, int rounds,
                       std::vector<uint8_t>* inlier_mask = nullptr);
    // find, the polish and the pose selection (erp_match.h "pose selection"; no reference
    // counterpart): the cheirality vote over (R1 | R2) x (+t | -t) on the polish's E and inlier
    // set.  R_vec_out / T_vec_out: the pose record's -- the reference's candidates made definite
    // (zeros when no match could vote: last_pose().status is then ERP_TOO_FEW_POINTS).
    // inlier_mask, depth ((d_l, d_r) per match) and front (may be nullptr) are resized to
    // match_size (depth: 2 * match_size).  Draws from the stream as find does.
    void find_posed(int im_width, int im_height, std::vector<KeyPoint>& key_left,
                    std::vector<KeyPoint>& key_right, Vec3f& R_vec_out, Vec3f& T_vec_out,
                    int match_size, float thr, int rounds, double min_sin2 = 0.0,
                    std::vector<uint8_t>* inlier_mask = nullptr,
                    std::vector<double>* depth = nullptr, std::vector<uint8_t>* front = nullptr);
    // find plus the winning iteration's record (erp_match.h "winner records"; no reference
    // counterpart): winner.E is the solved 9-vector R_vec_out / T_vec_out were decomposed from,
    // e.g. for an epipolar drawing of the returned pose.  Draws from the stream as find does.
    void find_winner(int im_width, int im_height, std::vector<KeyPoint>& key_left,
                     std::vector<KeyPoint>& key_right, Vec3f& R_vec_out, Vec3f& T_vec_out,
                     int match_size, erp_winner& winner);
    // find plus the support stage (erp_match.h "support-scored winner"; no reference
    // counterpart): R_vec_out / T_vec_out are the rotation and T of the scored iteration most
    // matches agree with under |l^T E' r| < thr, winner.E its solved 9-vector; last_result() is
    // find's own record (the consensus winner).  counts (optional) gets every iteration's
    // inlier count.  Pays with minimal samples (cfg.sample_frac for ~10 rows), not at the
    // reference's 0.25.  Draws from the stream as find does.
    void find_support(int im_width, int im_height, std::vector<KeyPoint>& key_left,
                      std::vector<KeyPoint>& key_right, Vec3f& R_vec_out, Vec3f& T_vec_out,
                      int match_size, float thr, erp_support& support, erp_winner& winner,
                      std::vector<int32_t>* counts = nullptr);
    // src/eight_point.hpp:15-19
    void eight_point_estimation(int im_width, int im_height, std::vector<Point3d>& key_point_left_rect,
                                std::vector<Point3d>& key_point_right_rect, Vec3f& R1_vec,
                                Vec3f& R2_vec, Vec3f& T_vec, bool& R1_valid, bool& R2_valid,
                                int match_size);
    // src/eight_point.hpp:20-23
    void initial_guess(int im_width, int im_height, std::vector<Point3d>& key_point_left_rect,
                       std::vector<Point3d>& key_point_right_rect, Vec3f& R_vec_out,
                       Vec3f& T_vec_out, int match_size);

    // Draw from `s` and advance it, as the reference's finds share the process-global rand()
    // (nullptr, the default: every call starts at cfg.seed / cfg.offset).  The stream must
    // outlive this object or be detached first.  The reference's semantics in one line:
    //   ep.use_stream(&erp::rand_stream::process());
    void use_stream(rand_stream* s);

    erp_ransac_cfg cfg;                 // reference constants (erp_ransac_cfg_default)
    const erp_pair_result& last_result() const { return last_; }
    const erp_polish_result& last_polish() const { return last_polish_; }
    const erp_pose& last_pose() const { return last_pose_; }

private:
    erp_ctx* ctx_ = nullptr;
    erp_pair_result last_{};
    erp_polish_result last_polish_{};
    erp_pose last_pose_{};
};

}  // namespace erp

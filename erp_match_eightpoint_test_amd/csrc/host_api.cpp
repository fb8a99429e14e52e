// host_api.cpp -- the C++ class API (include/erp/*.hpp) over the C ABI.  Host code only.
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/erp/eight_point.hpp"
#include "../../include/erp/feature_matcher.hpp"
#include "../../include/erp/rand_stream.hpp"

namespace erp {

static void check(erp_status s, const char* where) {
    if (s != ERP_OK) throw error(s, where);
}

feature_matcher::feature_matcher(int device) { check(erp_ctx_create(device, &ctx_), "feature_matcher"); }
feature_matcher::~feature_matcher() {
    if (ctx_) erp_ctx_destroy(ctx_);
}

// the rows of d back to back (d itself when it is packed already)
static const float* pack(const Descriptors& d, std::vector<float>& buf) {
    const size_t row = (size_t)d.cols * sizeof(float);
    if (d.step == 0 || d.step == row) return d.data;
    buf.resize((size_t)d.rows * d.cols);
    for (int r = 0; r < d.rows; r++)
        memcpy(&buf[(size_t)r * d.cols], (const char*)d.data + (size_t)r * d.step, row);
    return buf.data();
}

static std::vector<DMatch> to_dmatches(const std::vector<erp_dmatch>& out, int32_t n) {
    std::vector<DMatch> res((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        res[i].queryIdx = out[i].queryIdx;
        res[i].trainIdx = out[i].trainIdx;
        res[i].imgIdx = out[i].imgIdx;
        res[i].distance = out[i].distance;
    }
    return res;
}

std::vector<DMatch> feature_matcher::match_guided(const Descriptors& d1, const Descriptors& d2,
                                                  const std::vector<KeyPoint>& key1,
                                                  const std::vector<KeyPoint>& key2, int im_width,
                                                  int im_height, const double E[9], float thr,
                                                  float ratio, float max_dist, bool unique) {
    if (d1.cols != 64 || d2.cols != 64 || d1.rows < 0 || d2.rows < 0 ||
        key1.size() != (size_t)d1.rows || key2.size() != (size_t)d2.rows)
        throw error(ERP_INVALID_ARG, "match_guided: descriptors [n][64] with one keypoint per row");
    std::vector<float> b1, b2;
    const float* p1 = pack(d1, b1);
    const float* p2 = pack(d2, b2);
    std::vector<erp_point2f> k1(key1.size()), k2(key2.size());
    for (size_t i = 0; i < key1.size(); i++) k1[i] = erp_point2f{key1[i].pt.x, key1[i].pt.y};
    for (size_t i = 0; i < key2.size(); i++) k2[i] = erp_point2f{key2[i].pt.x, key2[i].pt.y};
    std::vector<erp_dmatch> out((size_t)std::max(d1.rows, 1));
    int32_t n = 0;
    const erp_guided_cfg cfg{thr, ratio, max_dist, unique ? 1 : 0};
    check(erp_match_guided(ctx_, p1, d1.rows, p2, d2.rows, k1.data(), k2.data(), im_width,
                           im_height, E, &cfg, out.data(), &n),
          "match_guided");
    return to_dmatches(out, n);
}

std::vector<DMatch> feature_matcher::match_two_image(const Descriptors& d1, const Descriptors& d2) {
    if (d1.cols != d2.cols) throw error(ERP_INVALID_ARG, "match_two_image: descriptor size");
    std::vector<float> b1, b2;
    const float* p1 = pack(d1, b1);
    const float* p2 = pack(d2, b2);
    std::vector<erp_dmatch> out((size_t)std::max(d1.rows, 1));
    int32_t n = 0;
    erp_status s;
    if (ratio_thresh == 0.3f) {
        s = erp_match_two_image(ctx_, p1, d1.rows, p2, d2.rows, d1.cols, out.data(), &n);
    } else {
        s = ERP_INVALID_ARG;  // the host entry point fixes the reference ratio
    }
    check(s, "match_two_image");
    return to_dmatches(out, n);
}

eight_point::eight_point(int device) {
    erp_ransac_cfg_default(&cfg);
    check(erp_ctx_create(device, &ctx_), "eight_point");
}
eight_point::~eight_point() {
    if (ctx_) erp_ctx_destroy(ctx_);
}

void eight_point::use_stream(rand_stream* s) {
    check(erp_ctx_set_rand_stream(ctx_, s ? s->handle() : nullptr), "use_stream");
}

// the first match_size keypoints of each side as the C ABI takes them; `where` names the check
static void keys(const std::vector<KeyPoint>& kl, const std::vector<KeyPoint>& kr, int match_size,
                 const char* where, std::vector<erp_point2f>& a, std::vector<erp_point2f>& b) {
    if (match_size < 0 || (size_t)match_size > kl.size() || (size_t)match_size > kr.size())
        throw error(ERP_INVALID_ARG, where);
    a.resize((size_t)match_size);
    b.resize((size_t)match_size);
    for (int i = 0; i < match_size; i++) {
        a[i] = erp_point2f{kl[i].pt.x, kl[i].pt.y};
        b[i] = erp_point2f{kr[i].pt.x, kr[i].pt.y};
    }
}

void eight_point::find(int W, int H, std::vector<KeyPoint>& kl, std::vector<KeyPoint>& kr,
                       Vec3f& R, Vec3f& T, int match_size) {
    std::vector<erp_point2f> a, b;
    keys(kl, kr, match_size, "find: match_size", a, b);
    check(erp_eight_point_find(ctx_, W, H, a.data(), b.data(), match_size, &cfg, R.val, T.val, &last_),
          "find");
}

void eight_point::find_winner(int W, int H, std::vector<KeyPoint>& kl, std::vector<KeyPoint>& kr,
                              Vec3f& R, Vec3f& T, int match_size, erp_winner& winner) {
    std::vector<erp_point2f> a, b;
    keys(kl, kr, match_size, "find_winner: match_size", a, b);
    check(erp_eight_point_find_winner(ctx_, W, H, a.data(), b.data(), match_size, &cfg, R.val,
                                      T.val, &last_, &winner),
          "find_winner");
    check((erp_status)winner.status, "find_winner: winner record");
}

void eight_point::find_support(int W, int H, std::vector<KeyPoint>& kl, std::vector<KeyPoint>& kr,
                               Vec3f& R, Vec3f& T, int match_size, float thr, erp_support& support,
                               erp_winner& winner, std::vector<int32_t>* counts) {
    std::vector<erp_point2f> a, b;
    keys(kl, kr, match_size, "find_support: match_size", a, b);
    if (counts) counts->assign((size_t)(cfg.iters > 0 ? cfg.iters : 0), 0);
    check(erp_eight_point_find_support(ctx_, W, H, a.data(), b.data(), match_size, &cfg, thr, R.val,
                                       T.val, &last_, &support, &winner, nullptr,
                                       counts && !counts->empty() ? counts->data() : nullptr),
          "find_support");
    check((erp_status)support.status, "find_support: support record");
}

void eight_point::find_polished(int W, int H, std::vector<KeyPoint>& kl, std::vector<KeyPoint>& kr,
                                Vec3f& R, Vec3f& T, int match_size, float thr, int rounds,
                                std::vector<uint8_t>* inlier_mask) {
    std::vector<erp_point2f> a, b;
    keys(kl, kr, match_size, "find_polished: match_size", a, b);
    if (inlier_mask) inlier_mask->assign((size_t)match_size, 0);
    check(erp_eight_point_find_polished(ctx_, W, H, a.data(), b.data(), match_size, &cfg, thr,
                                        rounds, &last_, &last_polish_,
                                        inlier_mask && match_size > 0 ? inlier_mask->data() : nullptr),
          "find_polished");
    for (int k = 0; k < 3; k++) {
        R[k] = last_polish_.R[k];
        T[k] = last_polish_.T[k];
    }
}

void eight_point::find_posed(int W, int H, std::vector<KeyPoint>& kl, std::vector<KeyPoint>& kr,
                             Vec3f& R, Vec3f& T, int match_size, float thr, int rounds,
                             double min_sin2, std::vector<uint8_t>* inlier_mask,
                             std::vector<double>* depth, std::vector<uint8_t>* front) {
    std::vector<erp_point2f> a, b;
    keys(kl, kr, match_size, "find_posed: match_size", a, b);
    if (inlier_mask) inlier_mask->assign((size_t)match_size, 0);
    if (depth) depth->assign((size_t)match_size * 2, 0.0);
    if (front) front->assign((size_t)match_size, 0);
    const bool any = match_size > 0;
    check(erp_eight_point_find_posed(ctx_, W, H, a.data(), b.data(), match_size, &cfg, thr, rounds,
                                     min_sin2, &last_, &last_polish_, &last_pose_,
                                     inlier_mask && any ? inlier_mask->data() : nullptr,
                                     depth && any ? depth->data() : nullptr,
                                     front && any ? front->data() : nullptr),
          "find_posed");
    for (int k = 0; k < 3; k++) {
        R[k] = last_pose_.R[k];
        T[k] = last_pose_.T[k];
    }
}

void eight_point::initial_guess(int, int, std::vector<Point3d>& l, std::vector<Point3d>& r, Vec3f& R,
                                Vec3f& T, int match_size) {
    if (match_size < 0 || (size_t)match_size > l.size() || (size_t)match_size > r.size())
        throw error(ERP_INVALID_ARG, "initial_guess: match_size");
    // (no &l[0] on an empty vector)
    const double* pl = match_size > 0 ? &l[0].x : nullptr;
    const double* pr = match_size > 0 ? &r[0].x : nullptr;
    check(erp_initial_guess(ctx_, pl, pr, match_size, &cfg, R.val, T.val, &last_), "initial_guess");
}

void eight_point::eight_point_estimation(int, int, std::vector<Point3d>& l, std::vector<Point3d>& r,
                                         Vec3f& R1, Vec3f& R2, Vec3f& T, bool& v1, bool& v2,
                                         int match_size) {
    if (match_size < 0 || (size_t)match_size > l.size() || (size_t)match_size > r.size())
        throw error(ERP_INVALID_ARG, "eight_point_estimation: match_size");
    erp_hypothesis h;
    const double* pl = match_size > 0 ? &l[0].x : nullptr;
    const double* pr = match_size > 0 ? &r[0].x : nullptr;
    check(erp_eight_point_estimation(ctx_, pl, pr, match_size, &h), "eight_point_estimation");
    for (int k = 0; k < 3; k++) {
        R1[k] = h.R1[k];
        R2[k] = h.R2[k];
        T[k] = h.T[k];
    }
    v1 = h.R1_valid != 0;
    v2 = h.R2_valid != 0;
}

rand_stream::rand_stream(uint32_t seed, uint64_t offset) {
    check(erp_rand_stream_create(seed, offset, &s_), "rand_stream");
}
rand_stream::rand_stream(process_tag, int device) : owned_(false) {
    check(erp_rand_stream_process(device, &s_), "rand_stream::process");
}
rand_stream::~rand_stream() {
    if (s_ && owned_) erp_rand_stream_destroy(s_);
}
rand_stream& rand_stream::process(int device) {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<rand_stream>> streams;
    std::lock_guard<std::mutex> g(mu);
    std::unique_ptr<rand_stream>& p = streams[device];
    if (!p) p.reset(new rand_stream(process_tag{}, device));
    return *p;
}
void rand_stream::get(uint32_t& seed, uint64_t& draws) const {
    check(erp_rand_stream_get(s_, &seed, &draws), "rand_stream::get");
}
uint64_t rand_stream::draws() const {
    uint32_t seed = 0;
    uint64_t d = 0;
    get(seed, d);
    return d;
}
void rand_stream::set(uint32_t seed, uint64_t offset) {
    check(erp_rand_stream_set(s_, seed, offset), "rand_stream::set");
}
void rand_stream::advance(uint64_t n) { check(erp_rand_stream_advance(s_, n), "rand_stream::advance"); }

}  // namespace erp

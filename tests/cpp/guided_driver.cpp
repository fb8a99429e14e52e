// A reference-side C++ program on the class API alone (include/erp/*.hpp): one
// erp::feature_matcher::match_guided (erp_match.h "guided matching").
//
//   guided_driver <in_dir> <out_dir>
// in:  meta.i32 = {W, H, n1, n2, unique}; cfg.f32 = {thr, ratio, max_dist}; e.f64 [9];
//      d1.f32 [n1][64], d2.f32 [n2][64], k1.f32 [n1][2], k2.f32 [n2][2]
// out: matches.bin (cv::DMatch-shaped records: queryIdx, trainIdx, imgIdx, distance)
#include <erp/feature_matcher.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <class T>
static std::vector<T> read_all(const std::string& path, size_t n) {
    std::vector<T> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "read %s failed\n", path.c_str());
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static void write_all(const std::string& path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) {
        std::fprintf(stderr, "write %s failed\n", path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in_dir> <out_dir>\n", argv[0]);
        return 2;
    }
    const std::string in = argv[1], out = argv[2];
    const std::vector<int> meta = read_all<int>(in + "/meta.i32", 5);
    const int W = meta[0], H = meta[1], n1 = meta[2], n2 = meta[3], unique = meta[4];
    const std::vector<float> cfg = read_all<float>(in + "/cfg.f32", 3);
    const std::vector<double> e = read_all<double>(in + "/e.f64", 9);
    const std::vector<float> d1 = read_all<float>(in + "/d1.f32", (size_t)n1 * 64);
    const std::vector<float> d2 = read_all<float>(in + "/d2.f32", (size_t)n2 * 64);
    const std::vector<float> p1 = read_all<float>(in + "/k1.f32", (size_t)n1 * 2);
    const std::vector<float> p2 = read_all<float>(in + "/k2.f32", (size_t)n2 * 2);
    std::vector<erp::KeyPoint> k1(n1), k2(n2);
    for (int k = 0; k < n1; k++) k1[k].pt = {p1[2 * k], p1[2 * k + 1]};
    for (int k = 0; k < n2; k++) k2[k].pt = {p2[2 * k], p2[2 * k + 1]};
    try {
        erp::feature_matcher matcher(0);
        erp::Descriptors q, t;
        q.data = d1.data();
        q.rows = n1;
        t.data = d2.data();
        t.rows = n2;
        const std::vector<erp::DMatch> m = matcher.match_guided(q, t, k1, k2, W, H, e.data(), cfg[0],
                                                                cfg[1], cfg[2], unique != 0);
        static_assert(sizeof(erp::DMatch) == 16, "cv::DMatch layout");
        write_all(out + "/matches.bin", m.data(), m.size() * sizeof(erp::DMatch));
    } catch (const erp::error& err) {
        std::fprintf(stderr, "erp::error %d: %s\n", (int)err.status, err.what());
        return 3;
    }
    std::printf("ok\n");
    return 0;
}

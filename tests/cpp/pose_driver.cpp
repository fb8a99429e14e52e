// A reference-side C++ program on the class API alone (include/erp/*.hpp): one
// erp::eight_point::find_posed -- find, the polish and the pose selection (erp_match.h "pose
// selection").
//
//   pose_driver <in_dir> <out_dir>
// in:  meta.i32 = {W, H, iters, m, rounds}; thr.f32 = {thr}; min_sin2.f64 = {min_sin2};
//      kl.f32 / kr.f32 [m][2]
// out: posed.bin (R, T as 6 floats + erp_pair_result + erp_polish_result + erp_pose), mask.u8 [m],
//      depth.f64 [m][2], front.u8 [m]
#include <erp/eight_point.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    const int W = meta[0], H = meta[1], iters = meta[2], m = meta[3], rounds = meta[4];
    const float thr = read_all<float>(in + "/thr.f32", 1)[0];
    const double min_sin2 = read_all<double>(in + "/min_sin2.f64", 1)[0];
    const std::vector<float> pl = read_all<float>(in + "/kl.f32", (size_t)m * 2);
    const std::vector<float> pr = read_all<float>(in + "/kr.f32", (size_t)m * 2);
    std::vector<erp::KeyPoint> kl(m), kr(m);
    for (int k = 0; k < m; k++) {
        kl[k].pt = {pl[2 * k], pl[2 * k + 1]};
        kr[k].pt = {pr[2 * k], pr[2 * k + 1]};
    }
    try {
        erp::eight_point estimater(0);
        estimater.cfg.iters = iters;
        erp::Vec3f R, T;
        std::vector<uint8_t> mask, front;
        std::vector<double> depth;
        estimater.find_posed(W, H, kl, kr, R, T, m, thr, rounds, min_sin2, &mask, &depth, &front);
        std::vector<char> buf(24 + sizeof(erp_pair_result) + sizeof(erp_polish_result) +
                              sizeof(erp_pose));
        char* w = buf.data();
        std::memcpy(w, R.val, 12);
        std::memcpy(w + 12, T.val, 12);
        w += 24;
        std::memcpy(w, &estimater.last_result(), sizeof(erp_pair_result));
        w += sizeof(erp_pair_result);
        std::memcpy(w, &estimater.last_polish(), sizeof(erp_polish_result));
        w += sizeof(erp_polish_result);
        std::memcpy(w, &estimater.last_pose(), sizeof(erp_pose));
        write_all(out + "/posed.bin", buf.data(), buf.size());
        write_all(out + "/mask.u8", mask.data(), mask.size());
        write_all(out + "/depth.f64", depth.data(), depth.size() * sizeof(double));
        write_all(out + "/front.u8", front.data(), front.size());
    } catch (const erp::error& e) {
        std::fprintf(stderr, "erp::error %d: %s\n", (int)e.status, e.what());
        return 3;
    }
    std::printf("ok\n");
    return 0;
}

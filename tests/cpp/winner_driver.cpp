// A reference-side C++ program on the class API alone (include/erp/*.hpp): one
// erp::eight_point::find_winner -- find plus the winning iteration's record (erp_match.h
// "winner records").
//
//   winner_driver <in_dir> <out_dir>
// in:  meta.i32 = {W, H, iters, m}; kl.f32 / kr.f32 [m][2]
// out: winner.bin (R, T as 6 floats + erp_pair_result + erp_winner)
#include <erp/eight_point.hpp>

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

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in_dir> <out_dir>\n", argv[0]);
        return 2;
    }
    const std::string in = argv[1], out = argv[2];
    const std::vector<int> meta = read_all<int>(in + "/meta.i32", 4);
    const int W = meta[0], H = meta[1], iters = meta[2], m = meta[3];
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
        erp_winner w;
        estimater.find_winner(W, H, kl, kr, R, T, m, w);
        std::vector<char> buf(24 + sizeof(erp_pair_result) + sizeof(erp_winner));
        std::memcpy(buf.data(), R.val, 12);
        std::memcpy(buf.data() + 12, T.val, 12);
        std::memcpy(buf.data() + 24, &estimater.last_result(), sizeof(erp_pair_result));
        std::memcpy(buf.data() + 24 + sizeof(erp_pair_result), &w, sizeof(w));
        const std::string path = out + "/winner.bin";
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(buf.data(), 1, buf.size(), f) != buf.size()) {
            std::fprintf(stderr, "write %s failed\n", path.c_str());
            return 2;
        }
        std::fclose(f);
    } catch (const erp::error& e) {
        std::fprintf(stderr, "erp::error %d: %s\n", (int)e.status, e.what());
        return 3;
    }
    std::printf("ok\n");
    return 0;
}

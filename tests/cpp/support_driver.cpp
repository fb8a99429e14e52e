// A reference-side C++ program on the class API alone (include/erp/*.hpp): one
// erp::eight_point::find_support -- find plus the support stage (erp_match.h "support-scored
// winner").
//
//   support_driver <in_dir> <out_dir>
// in:  meta.i32 = {W, H, iters, m}; cfg.f64 = {sample_frac, thr}; kl.f32 / kr.f32 [m][2]
// out: support.bin (R, T as 6 floats + erp_pair_result + erp_support + erp_winner +
//      counts [iters] int32)
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
    const std::vector<double> cf = read_all<double>(in + "/cfg.f64", 2);
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
        estimater.cfg.sample_frac = cf[0];
        erp::Vec3f R, T;
        erp_support s;
        erp_winner w;
        std::vector<int32_t> counts;
        estimater.find_support(W, H, kl, kr, R, T, m, (float)cf[1], s, w, &counts);
        std::vector<char> buf(24 + sizeof(erp_pair_result) + sizeof(s) + sizeof(w) +
                              counts.size() * sizeof(int32_t));
        char* o = buf.data();
        std::memcpy(o, R.val, 12);
        std::memcpy(o + 12, T.val, 12);
        o += 24;
        std::memcpy(o, &estimater.last_result(), sizeof(erp_pair_result));
        o += sizeof(erp_pair_result);
        std::memcpy(o, &s, sizeof(s));
        o += sizeof(s);
        std::memcpy(o, &w, sizeof(w));
        o += sizeof(w);
        std::memcpy(o, counts.data(), counts.size() * sizeof(int32_t));
        const std::string path = out + "/support.bin";
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

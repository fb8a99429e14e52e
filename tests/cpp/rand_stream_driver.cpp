// A reference-side C++ program on the class API alone (include/erp/*.hpp): a fresh
// erp::eight_point per iteration, as the reference's drivers build a fresh `estimater` in their
// loops (one_image_test/main.cpp:135-137, two_real_image_test/main.cpp:283-286), all drawing
// from the process-wide rand stream -- the reference's process-global rand().
//
//   rand_stream_driver <in_dir> <out_dir>
// in:  meta.i32 = {W, H, iters, n_sets, m_0, .., m_{n_sets-1}}; kl<i>.f32 / kr<i>.f32 [m_i][2]
// out: find<i>.bin (R, T as 6 floats + erp_pair_result), draws.u64 [n_sets + 1] (the stream's
//      counter before the first find and after each)
#include <erp/eight_point.hpp>
#include <erp/rand_stream.hpp>

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
    const std::vector<int> head = read_all<int>(in + "/meta.i32", 4);
    const int W = head[0], H = head[1], iters = head[2], n_sets = head[3];
    const std::vector<int> meta = read_all<int>(in + "/meta.i32", 4 + (size_t)n_sets);
    try {
        erp::rand_stream& rs = erp::rand_stream::process();
        std::vector<uint64_t> draws{rs.draws()};
        for (int i = 0; i < n_sets; i++) {
            const int m = meta[4 + i];
            const std::vector<float> pl = read_all<float>(in + "/kl" + std::to_string(i) + ".f32", (size_t)m * 2);
            const std::vector<float> pr = read_all<float>(in + "/kr" + std::to_string(i) + ".f32", (size_t)m * 2);
            std::vector<erp::KeyPoint> kl(m), kr(m);
            for (int k = 0; k < m; k++) {
                kl[k].pt = {pl[2 * k], pl[2 * k + 1]};
                kr[k].pt = {pr[2 * k], pr[2 * k + 1]};
            }
            erp::eight_point estimater(0);
            estimater.cfg.iters = iters;
            estimater.use_stream(&rs);  // the one line that turns the reference's semantics on
            erp::Vec3f R, T;
            estimater.find(W, H, kl, kr, R, T, m);
            std::vector<char> buf(6 * sizeof(float) + sizeof(erp_pair_result));
            std::memcpy(buf.data(), R.val, 12);
            std::memcpy(buf.data() + 12, T.val, 12);
            std::memcpy(buf.data() + 24, &estimater.last_result(), sizeof(erp_pair_result));
            write_all(out + "/find" + std::to_string(i) + ".bin", buf.data(), buf.size());
            draws.push_back(rs.draws());
        }
        write_all(out + "/draws.u64", draws.data(), draws.size() * sizeof(uint64_t));
    } catch (const erp::error& e) {
        std::fprintf(stderr, "erp::error %d: %s\n", (int)e.status, e.what());
        return 3;
    }
    std::printf("ok\n");
    return 0;
}

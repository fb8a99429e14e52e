// A C++ program on the C ABI alone (include/erp_match.h "dense stereo on row-rectified views"):
// one erp_stereo_rows_ex_dev call (eight paths, uniqueness) on images read from files, as a
// reference maintainer links it.
//
//   stereo_ex_driver <in_dir> <out_dir>
// in:  meta.i32 = {n_pairs, rows, cols, d_min, n_disp, p1, p2, lr_max, wrap_rows, channels,
//                  n_paths, uniqueness};
//      left.u8 / right.u8 [n_pairs][rows][cols][channels]
// out: disp16.i16 [n_pairs][rows][cols], depth.f32 [n_pairs][rows][cols]
#include <erp_match.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// the four HIP runtime calls the program needs (libamdhip64), declared here so that it builds
// with the host compiler and no HIP headers
extern "C" {
int hipMalloc(void** ptr, size_t bytes);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);  // 1 = H2D, 2 = D2H
int hipDeviceSynchronize(void);
}

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

static void* to_device(const void* h, size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != 0 || (h && hipMemcpy(d, h, bytes, 1) != 0)) {
        std::fprintf(stderr, "device allocation or copy of %zu bytes failed\n", bytes);
        std::exit(2);
    }
    return d;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in_dir> <out_dir>\n", argv[0]);
        return 2;
    }
    const std::string in = argv[1], out = argv[2];
    const std::vector<int> m = read_all<int>(in + "/meta.i32", 12);
    const int n = m[0], rows = m[1], cols = m[2];
    erp_stereo_params_ex ex;
    erp_stereo_params_ex_default(&ex);
    erp_stereo_params& p = ex.base;
    ex.n_paths = m[10], ex.uniqueness = m[11];
    p.d_min = m[3], p.n_disp = m[4], p.p1 = m[5], p.p2 = m[6], p.lr_max = m[7];
    p.wrap_rows = m[8], p.channels = m[9];
    const size_t px = (size_t)n * rows * cols;
    const std::vector<uint8_t> left = read_all<uint8_t>(in + "/left.u8", px * p.channels);
    const std::vector<uint8_t> right = read_all<uint8_t>(in + "/right.u8", px * p.channels);
    erp_ctx* ctx = nullptr;
    erp_status s = erp_ctx_create(0, &ctx);
    if (s != ERP_OK) {
        std::fprintf(stderr, "erp_ctx_create: %s\n", erp_status_string(s));
        return 3;
    }
    void* d_left = to_device(left.data(), left.size());
    void* d_right = to_device(right.data(), right.size());
    void* d_disp = to_device(nullptr, px * 2);
    void* d_depth = to_device(nullptr, px * 4);
    s = erp_stereo_rows_ex_dev(ctx, (const uint8_t*)d_left, (const uint8_t*)d_right, n, rows, cols,
                               &ex, (int16_t*)d_disp, (float*)d_depth, nullptr);
    if (s != ERP_OK || hipDeviceSynchronize() != 0) {
        std::fprintf(stderr, "erp_stereo_rows_ex_dev: %s\n", erp_status_string(s));
        return 3;
    }
    std::vector<int16_t> disp(px);
    std::vector<float> depth(px);
    if (hipMemcpy(disp.data(), d_disp, px * 2, 2) != 0 ||
        hipMemcpy(depth.data(), d_depth, px * 4, 2) != 0) {
        std::fprintf(stderr, "copy back failed\n");
        return 3;
    }
    write_all(out + "/disp16.i16", disp.data(), px * 2);
    write_all(out + "/depth.f32", depth.data(), px * 4);
    hipFree(d_left), hipFree(d_right), hipFree(d_disp), hipFree(d_depth);
    erp_ctx_destroy(ctx);
    std::printf("ok\n");
    return 0;
}

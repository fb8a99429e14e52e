// stereo.hip -- dense disparity on row-rectified views (include/erp_match.h "dense stereo on
// row-rectified views"; no reference counterpart): census + 4-path SGM, the winner with its
// sub-pixel offset, the left-right check and the optional depth.  The header states the rules;
// every kernel below restates its rule in integers, so the output is the rules' bit for bit.
//
// Scratch of a chunk of n pairs (rows x cols, D disparities):
//   census   [2][n][rows][cols] u64   the left images' words, then the right images'
//   S        [n][rows][cols][D] u16   d innermost: a pixel's D sums are D * 2 contiguous bytes
//   winners  [2][n][rows][cols] i16   d*, then dR (-1 where no d has its column in range)
// Its launches:
//   census   256 threads per 64 x 4 tile of one image; the tile's gray values with the 4-column /
//            3-row halo go through LDS (columns clamped, rows wrapped or clamped while loading).
//   paths    twice, along rows and along columns.  A lane owns 4 consecutive disparities (one
//            8-byte word of S), a group of WIDTH = 4..64 lanes owns a line's D, a wave owns
//            64 / WIDTH neighbouring lines and walks them forwards, then backwards.  The cost is
//            computed on the way from the two census words (__popcll) and never stored; the L of
//            the previous pixel stays in registers; its minimum over d is taken over the group's
//            lanes on DPP (group_min), d-1 / d+1 across the lanes' borders are one DPP wave shift
//            each.  Four u16 sums add as one 64-bit integer (S <= 1272 per field: no carry
//            crosses a field).  The horizontal launch's forward walk stores S, every other walk
//            adds to it; each lane only ever touches its own words, so there are no atomics and
//            the sum's order is fixed.  A walk is one dependent chain per wave, so the words of
//            the next kPathAhead pixels are loaded ahead of a pixel's recurrence, without
//            branches; 4 ahead is enough (8 measured the same: what is left is the instruction
//            count per pixel).  Along rows a wave's lines are 64 / WIDTH rows (one
//            S row of D * 2 bytes each per step); along columns they are neighbouring columns,
//            whose S rows are contiguous.
//   winner   a block per 1024-column segment of a row, a group per column: the first argmin of
//            S(y,x,.) with the parabola offset, and dR by an LDS minimum over the segment's
//            right-image pixels, so that S is read in rows here too (comment at the kernel).
//   check    one lane per pixel: rule 6 in place on disp16, rule 7.
// D > 64 needs no second wave: 64 lanes x 4 disparities cover the largest D (256).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/erp_match.h"
#include "erp_ctx.hpp"
#include "erp_launch.hpp"

namespace erp {

namespace {

constexpr int kCenTW = 64, kCenTH = 4;          // census tile: 64 columns x 4 rows
constexpr int kCenLW = kCenTW + 8, kCenLH = kCenTH + 6;
#ifndef ERP_STEREO_PATH_AHEAD
#define ERP_STEREO_PATH_AHEAD 4
#endif
constexpr int kPathAhead = ERP_STEREO_PATH_AHEAD;  // pixels whose words a path walk keeps in flight
constexpr int kWinT = 1024;                      // columns of a winner block's segment
constexpr int kBig = 1 << 20;                    // an L no minimum ever takes
constexpr int kMaxChunkPairs = 16384;            // grid.y: 2 n images or n pairs
constexpr int64_t kMaxPixels = (int64_t)1 << 30;

struct StereoArgs {
    const uint8_t* left;
    const uint8_t* right;
    uint64_t* census;   // [2][n][rows][cols]
    uint16_t* S;        // [n][rows][cols][D]
    int16_t* dstar;     // [n][rows][cols]
    int16_t* dright;    // [n][rows][cols]
    int16_t* disp16;    // the caller's, at the chunk's first pair
    float* depth;       // the caller's, at the chunk's first pair, or nullptr
    int n, rows, cols, D, d_min, p1, p2, lr_max, wrap, channels;
};

// ---------------------------------------------------------------------------- census ----
__global__ __launch_bounds__(256) void stereo_census_kernel(StereoArgs a) {
    __shared__ uint8_t g[kCenLH][kCenLW];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int rows = a.rows, cols = a.cols, ch = a.channels;
    const int tiles_x = (cols + kCenTW - 1) / kCenTW;  // (grid.x: the tiles in row-major order)
    const int x0 = (blockIdx.x % tiles_x) * kCenTW, y0 = (blockIdx.x / tiles_x) * kCenTH;
    const size_t px = (size_t)rows * cols;
    const uint8_t* src = (img < a.n ? a.left + (size_t)img * px * ch
                                    : a.right + (size_t)(img - a.n) * px * ch);
    for (int i = tid; i < kCenLH * kCenLW; i += 256) {
        const int ty = i / kCenLW, tx = i - ty * kCenLW;
        int gy = y0 + ty - 3, gx = x0 + tx - 4;
        gx = min(max(gx, 0), cols - 1);
        if (a.wrap) {
            gy %= rows;  // (any rows >= 1: the window may lap a short image more than once)
            if (gy < 0) gy += rows;
        } else {
            gy = min(max(gy, 0), rows - 1);
        }
        const uint8_t* p = src + ((size_t)gy * cols + gx) * ch;
        g[ty][tx] = ch == 3 ? (uint8_t)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + 8192) >> 14) : p[0];
    }
    __syncthreads();
    const int ty = tid >> 6, tx = tid & 63;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= rows || x >= cols) return;
    const int c = g[ty + 3][tx + 4];
    uint64_t w = 0;
    int k = 0;
#pragma unroll
    for (int dy = 0; dy < 7; dy++)
#pragma unroll
        for (int dx = 0; dx < 9; dx++) {
            if (dy == 3 && dx == 4) continue;
            w |= (uint64_t)(g[ty + dy][tx + dx] < c ? 1 : 0) << k;
            k++;
        }
    a.census[(size_t)img * px + (size_t)y * cols + x] = w;
}

// ----------------------------------------------------------------------------- paths ----
// what a lane needs of one pixel: the left word, its 4 right words (bit k of oob: disparity
// 4 gl + k has its column out of range) and, on an adding walk, its word of S
struct PathStep {
    uint64_t cl, cr[4], s;
    int oob;
};

// v of another lane through the DPP crossbar (all lanes are active where this is used)
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
constexpr int kDppXor1 = 0xb1, kDppXor2 = 0x4e;             // quad_perm [1,0,3,2], [2,3,0,1]
constexpr int kDppHalfMirror = 0x141, kDppMirror = 0x140;   // lane i <- 7 - i, 15 - i of its row
constexpr int kDppWaveShr1 = 0x138, kDppWaveShl1 = 0x130;   // lane i <- i - 1, i + 1 of the wave

// the minimum over each group of WIDTH lanes, in every lane: inside a row of 16 lanes on DPP (a
// quad's lanes agree after the two quad steps, so the mirrors that follow pair each lane with
// one of the other quad, then of the other half), across rows on the LDS crossbar
template <int WIDTH>
__device__ __forceinline__ int group_min(int m) {
    m = min(m, dpp_mov<kDppXor1>(m));
    m = min(m, dpp_mov<kDppXor2>(m));
    if (WIDTH >= 8) m = min(m, dpp_mov<kDppHalfMirror>(m));
    if (WIDTH >= 16) m = min(m, dpp_mov<kDppMirror>(m));
    if (WIDTH >= 32) m = min(m, __shfl_xor(m, 16, 64));
    if (WIDTH >= 64) m = min(m, __shfl_xor(m, 32, 64));
    return m;
}

template <int WIDTH, bool VERT>
__global__ __launch_bounds__(256) void stereo_path_kernel(StereoArgs a) {
    constexpr int LPW = 64 / WIDTH;  // lines of a wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = lane & (WIDTH - 1);
    const int rows = a.rows, cols = a.cols, D = a.D;
    const int n_lines = VERT ? cols : rows, len = VERT ? rows : cols;
    const int line0 = (blockIdx.x * 4 + wave) * LPW;
    if (line0 >= n_lines) return;  // (wave-uniform; the kernel has no block barrier)
    const int line = line0 + lane / WIDTH;
    const int d0 = 4 * gl;
    const int dq = D >> 2, d_min = a.d_min, p1 = a.p1, p2 = a.p2;
    const bool act = line < n_lines && d0 < D;  // (D is a multiple of 16: all 4 or none)
    // Every load below is unconditional, so that no branch stands between a load and its use and
    // the loads of kPathAhead pixels stay in flight: a lane that is not active reads what the
    // wave's last line, or its group's last word, reads (in bounds) and stores nothing.
    const int line_c = min(line, n_lines - 1), gl_c = min(gl, dq - 1);
    const size_t px = (size_t)rows * cols, pair = blockIdx.y;
    const uint64_t* cenL = a.census + pair * px;
    const uint64_t* cenR = a.census + ((size_t)a.n + pair) * px;
    uint64_t* S = (uint64_t*)(a.S + pair * px * D);  // a pixel's D / 4 words

    auto load = [&](int p, auto read_s) {
        PathStep st;
        const int y = VERT ? p : line_c, x = VERT ? line_c : p;
        const unsigned row = (unsigned)y * cols;  // (rows * cols <= 2^30: pixel indices fit 32 bits)
        st.cl = cenL[row + x];
        const int xr0 = x - d_min - d0;
        st.oob = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int xr = xr0 - k;
            st.cr[k] = cenR[row + min(max(xr, 0), cols - 1)];
            st.oob |= (xr < 0 || xr >= cols) ? 1 << k : 0;
        }
        st.s = decltype(read_s)::value ? S[(size_t)(row + x) * dq + gl_c] : 0;
        return st;
    };

    int L[4] = {kBig, kBig, kBig, kBig};
    // pixel p, the i-th of its walk, from its words
    auto step = [&](const PathStep& cur, int i, int p) {
        int c[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            c[k] = (cur.oob >> k) & 1 ? 63 : __popcll(cur.cl ^ cur.cr[k]);
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) L[k] = act ? c[k] : kBig;
        } else {
            const int m = group_min<WIDTH>(min(min(L[0], L[1]), min(L[2], L[3])));
            int below = dpp_mov<kDppWaveShr1>(L[3]), above = dpp_mov<kDppWaveShl1>(L[0]);
            if (gl == 0) below = kBig;           // d - 1 < 0: left out
            if (gl == WIDTH - 1) above = kBig;   // d + 1 >= D (a lane past D holds kBig)
            const int jump = m + p2;
            int n[4];
            n[0] = c[0] + min(min(L[0], min(below, L[1]) + p1), jump) - m;
            n[1] = c[1] + min(min(L[1], min(L[0], L[2]) + p1), jump) - m;
            n[2] = c[2] + min(min(L[2], min(L[1], L[3]) + p1), jump) - m;
            n[3] = c[3] + min(min(L[3], min(L[2], above) + p1), jump) - m;
#pragma unroll
            for (int k = 0; k < 4; k++) L[k] = act ? n[k] : kBig;
        }
        if (act) {
            const uint64_t pk = (uint64_t)(uint32_t)L[0] | ((uint64_t)(uint32_t)L[1] << 16) |
                                ((uint64_t)(uint32_t)L[2] << 32) | ((uint64_t)(uint32_t)L[3] << 48);
            const int y = VERT ? p : line, x = VERT ? line : p;
            S[(size_t)((unsigned)y * cols + x) * dq + gl] = cur.s + pk;  // (cur.s = 0 on the storing walk)
        }
    };
    // One walk, forwards (dir 0) or backwards.  The words of the next kPathAhead pixels are in
    // flight while a pixel's recurrence runs (a ring in registers: the loop is unrolled by its
    // length; past the walk's end the ring reloads the last pixel).  The backward walk of the
    // horizontal launch loads words this lane stored itself, earlier in program order.
    auto walk = [&](auto read_s, int dir) {
        auto at = [&](int i) { return dir ? len - 1 - min(i, len - 1) : min(i, len - 1); };
        PathStep ring[kPathAhead];
#pragma unroll
        for (int j = 0; j < kPathAhead; j++) ring[j] = load(at(j), read_s);
        for (int i0 = 0; i0 < len; i0 += kPathAhead) {
#pragma unroll
            for (int j = 0; j < kPathAhead; j++) {
                const int i = i0 + j;
                if (i >= len) break;
                const PathStep cur = ring[j];
                ring[j] = load(at(i + kPathAhead), read_s);
                step(cur, i, at(i));
            }
        }
    };
    if (VERT)
        walk(std::true_type{}, 0);
    else
        walk(std::false_type{}, 0);  // the first walk of the call stores S
    walk(std::true_type{}, 1);
}

// ---------------------------------------------------------------------------- winner ----
// A block owns segment k of a row: the kWinT columns from x0 = k kWinT for rule 5 and the
// kWinT right-image pixels from xr0 = x0 - d_min - D + 1 for dR.  It reads the S rows of the
// columns [x0 - D + 1, x0 + kWinT) once, in order, a group of WIDTH lanes per column: every sum
// S(y,x,d) is a candidate of xr = x - d_min - d, entry (x - x0) + (D - 1 - d) of the segment, and
// goes into an LDS minimum over the key (S << 16 | d), whose smallest value is the first argmin.
// The minimum does not depend on the order of its operands, so the LDS atomics keep the call
// deterministic.  k runs over every segment that holds a column or a right-image pixel of the
// image (the launch's kmin, grid.x); the columns left of x0 are read by two blocks.
template <int WIDTH>
__global__ __launch_bounds__(256) void stereo_winner_kernel(StereoArgs a, int kmin) {
    __shared__ uint32_t best[kWinT];
    constexpr int PPB = 256 / WIDTH;  // columns of a block's step
    const int tid = threadIdx.x, gl = tid & (WIDTH - 1), grp = tid / WIDTH;
    const int rows = a.rows, cols = a.cols, D = a.D;
    const size_t px = (size_t)rows * cols, pair = blockIdx.z;
    const int x0 = (kmin + (int)blockIdx.x) * kWinT, xr0 = x0 - a.d_min - D + 1;
    const int xs = max(x0 - D + 1, 0), xe = min(x0 + kWinT, cols);  // the columns read
    const int d0 = 4 * gl;
    const uint16_t* Sp = a.S + pair * px * D;
    for (int y = blockIdx.y; y < rows; y += gridDim.y) {
        for (int j = tid; j < kWinT; j += 256) best[j] = 0xffffffffu;
        __syncthreads();
        const size_t rowq = (size_t)y * cols;
        for (int xb = xs; xb < xe; xb += PPB) {  // (block-uniform bounds)
            const int x = xb + grp;
            const bool act = x < xe && d0 < D;
            int bv = 0xffff, bd = 0x7fff;
            if (act) {
                const uint64_t w = *(const uint64_t*)(Sp + (rowq + x) * D + d0);
                const int e0 = (x - x0) + (D - 1 - d0);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t v = (uint32_t)(w >> (16 * k)) & 0xffffu;
                    if ((int)v < bv) {  // rule 5: the first argmin of S(y,x,.)
                        bv = (int)v;
                        bd = d0 + k;
                    }
                    if ((unsigned)(e0 - k) < (unsigned)kWinT)
                        atomicMin(&best[e0 - k], (v << 16) | (uint32_t)(d0 + k));
                }
            }
            if (xb + PPB <= x0) continue;  // (block-uniform) columns read for dR alone
#pragma unroll
            for (int o = 1; o < WIDTH; o <<= 1) {
                const int ov = __shfl_xor(bv, o, 64), od = __shfl_xor(bd, o, 64);
                if (ov < bv || (ov == bv && od < bd)) {
                    bv = ov;
                    bd = od;
                }
            }
            if (gl != 0 || x < x0 || x >= xe) continue;
            const size_t q = rowq + x;
            int off = 0;
            if (bd > 0 && bd < D - 1) {
                const int sa = Sp[q * D + bd - 1], sb = Sp[q * D + bd + 1];
                const int den = sa + sb - 2 * bv;
                if (den > 0) {
                    const int num = (sa - sb) * 16 + den, d2 = 2 * den;
                    off = num >= 0 ? num / d2 : -((-num + d2 - 1) / d2);  // floor
                }
            }
            a.dstar[pair * px + q] = (int16_t)bd;
            a.disp16[pair * px + q] = (int16_t)(16 * (a.d_min + bd) + off);
        }
        __syncthreads();
        for (int j = tid; j < kWinT; j += 256) {
            const int xr = xr0 + j;
            if (xr < 0 || xr >= cols) continue;
            const uint32_t key = best[j];  // (untouched: no d has its column in range)
            a.dright[pair * px + rowq + xr] = (int16_t)(key == 0xffffffffu ? -1 : (int)(key & 0xffffu));
        }
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------- check ----
__global__ __launch_bounds__(256) void stereo_check_kernel(StereoArgs a) {
    const size_t px = (size_t)a.rows * a.cols, pair = blockIdx.y;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= px) return;
    const int cols = a.cols;
    const size_t row = q / cols;
    const int x = (int)(q - row * cols);
    const size_t o = pair * px + q;
    const int ds = a.dstar[o];
    const int xr = x - a.d_min - ds;
    bool valid = xr >= 0 && xr < cols;
    if (valid && a.lr_max >= 0) {
        const int dr = a.dright[pair * px + row * cols + xr];
        valid = abs(ds - dr) <= a.lr_max;
    }
    const int disp = a.disp16[o];
    if (!valid) a.disp16[o] = (int16_t)ERP_STEREO_INVALID;
    if (!a.depth) return;
    float z;
    if (!valid) {
        z = __builtin_nanf("");
    } else if (disp == 0) {
        z = __builtin_huge_valf();
    } else {
        const double thL = M_PI * (double)x / (double)cols;
        const double thR = M_PI * ((double)x - (double)disp / 16.0) / (double)cols;
        z = (float)(sin(thR) / fabs(sin(thL - thR)));
    }
    a.depth[o] = z;
}

template <int WIDTH>
hipError_t launch_chunk_w(const StereoArgs& a, hipStream_t st) {
    constexpr int LPB = 4 * (64 / WIDTH);  // lines of a path block
    const unsigned n = (unsigned)a.n;
    ERP_LAUNCH((stereo_path_kernel<WIDTH, false>), dim3((a.rows + LPB - 1) / LPB, n), dim3(256), 0,
               st, a);
    ERP_LAUNCH((stereo_path_kernel<WIDTH, true>), dim3((a.cols + LPB - 1) / LPB, n), dim3(256), 0,
               st, a);
    // the winner's segments: every k whose kWinT columns or kWinT right-image pixels (those
    // start d_min + D - 1 to the left of the columns) meet the image
    const int off = a.d_min + a.D - 1;
    const int kmin = std::min(0, off >= 0 ? off / kWinT : -((-off + kWinT - 1) / kWinT));
    const int kmax = (a.cols + std::max(off, 0) + kWinT - 1) / kWinT;
    ERP_LAUNCH((stereo_winner_kernel<WIDTH>),
               dim3((unsigned)(kmax - kmin), (unsigned)std::min(a.rows, 65535), n), dim3(256), 0, st,
               a, kmin);
    return hipGetLastError();
}

// one chunk: census, the two path launches, the winner and the check
hipError_t launch_chunk(const StereoArgs& a, hipStream_t st) {
    const unsigned n = (unsigned)a.n;
    const size_t px = (size_t)a.rows * a.cols;
    const size_t tiles = (size_t)((a.cols + kCenTW - 1) / kCenTW) * ((a.rows + kCenTH - 1) / kCenTH);
    ERP_LAUNCH(stereo_census_kernel, dim3((unsigned)tiles, 2 * n), dim3(256), 0, st, a);
    const int w = a.D / 4;  // lanes a line's D needs; the group is the power of two above
    hipError_t e;
    if (w <= 4)
        e = launch_chunk_w<4>(a, st);
    else if (w <= 8)
        e = launch_chunk_w<8>(a, st);
    else if (w <= 16)
        e = launch_chunk_w<16>(a, st);
    else if (w <= 32)
        e = launch_chunk_w<32>(a, st);
    else
        e = launch_chunk_w<64>(a, st);
    if (e != hipSuccess) return e;
    ERP_LAUNCH(stereo_check_kernel, dim3((unsigned)((px + 255) / 256), n), dim3(256), 0, st, a);
    return hipGetLastError();
}

bool params_ok(const erp_stereo_params& p) {
    if (p.n_disp < 16 || p.n_disp > 256 || p.n_disp % 16) return false;
    if (p.d_min < -2047 || p.d_min > 2047) return false;
    if ((p.d_min < 0 ? -p.d_min : p.d_min) + p.n_disp > 2047) return false;
    if (p.p1 < 0 || p.p1 > p.p2 || p.p2 > 255) return false;
    if (p.lr_max < -1) return false;
    if (p.wrap_rows != 0 && p.wrap_rows != 1) return false;
    return p.channels == 1 || p.channels == 3;
}

}  // namespace

}  // namespace erp

extern "C" {

void erp_stereo_params_default(erp_stereo_params* p) {
    if (!p) return;
    p->d_min = 0;
    p->n_disp = 64;
    p->p1 = 8;
    p->p2 = 64;
    p->lr_max = 1;
    p->wrap_rows = 0;
    p->channels = 3;
}

erp_status erp_stereo_rows_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                               int32_t n_pairs, int32_t rows, int32_t cols,
                               const erp_stereo_params* params, int16_t* d_disp16,
                               float* d_depth, void* stream) {
    if (!ctx || !params || n_pairs < 0 || rows < 1 || cols < 1 ||
        (int64_t)rows * cols > erp::kMaxPixels || !erp::params_ok(*params))
        return ERP_INVALID_ARG;
    if (n_pairs == 0) return ERP_OK;
    if (!d_left || !d_right || !d_disp16) return ERP_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return ERP_HIP_ERROR;
    hipStream_t st = (hipStream_t)stream;
    erp::CtxCall call(ctx, st);
    const size_t px = (size_t)rows * cols, D = (size_t)params->n_disp;
    const size_t vol = px * D * 2;  // one pair's S
    // the chunk: as many pairs as fit the option's MiB of S, at least one (include/erp_match.h)
    const size_t cap = (size_t)ctx->opt[ERP_OPT_STEREO_CHUNK_MB] << 20;
    const int chunk = (int)std::min<size_t>(std::max<size_t>(cap / vol, 1),
                                            std::min<size_t>(n_pairs, erp::kMaxChunkPairs));
    uint64_t* census = erp::ctx_scratch<uint64_t>(ctx, erp::kSlotStereoCensus, 2 * chunk * px * 8);
    uint16_t* S = erp::ctx_scratch<uint16_t>(ctx, erp::kSlotStereoVolume, chunk * vol);
    int16_t* win = erp::ctx_scratch<int16_t>(ctx, erp::kSlotStereoWinners, 2 * chunk * px * 2);
    if (!census || !S || !win) return ERP_OUT_OF_MEMORY;
    erp::StereoArgs a{};
    a.census = census;
    a.S = S;
    a.dstar = win;
    a.dright = win + chunk * px;
    a.rows = rows;
    a.cols = cols;
    a.D = params->n_disp;
    a.d_min = params->d_min;
    a.p1 = params->p1;
    a.p2 = params->p2;
    a.lr_max = params->lr_max;
    a.wrap = params->wrap_rows;
    a.channels = params->channels;
    for (int32_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        a.n = std::min(chunk, n_pairs - p0);
        a.left = d_left + (size_t)p0 * px * a.channels;
        a.right = d_right + (size_t)p0 * px * a.channels;
        a.disp16 = d_disp16 + (size_t)p0 * px;
        a.depth = d_depth ? d_depth + (size_t)p0 * px : nullptr;
        if (erp::launch_chunk(a, st) != hipSuccess) return ERP_HIP_ERROR;
    }
    return ERP_OK;
}

}  // extern "C"

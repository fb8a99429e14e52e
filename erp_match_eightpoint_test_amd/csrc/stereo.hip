// stereo.hip -- dense disparity on row-rectified views (include/erp_match.h "dense stereo on
// row-rectified views"; no reference counterpart): census + 4- or 8-path SGM, the winner with its
// sub-pixel offset, the left-right check, the optional uniqueness test and the optional depth.
// The header states the rules; every kernel below restates its rule in integers, so the output
// is the rules' bit for bit.
//
// Scratch of a chunk of n pairs (rows x cols, D disparities):
//   census   [2][n][rows][cols] u64   the left images' words, then the right images'
//   S        [n][rows][cols][D] u16   d innermost: a pixel's D sums are D * 2 contiguous bytes
//   winners  [2][n][rows][cols] i16   d* (bit 8: rule 6b rejected the pixel), then dR (-1 where
//                                     no d has its column in range)
// Its launches:
//   census   256 threads per 64 x 4 tile of one image; the tile's gray values with the 4-column /
//            3-row halo go through LDS (columns clamped, rows wrapped or clamped while loading).
//   paths    twice, along rows and along columns.  A lane owns 4 consecutive disparities (one
//            8-byte word of S), a group of WIDTH = 4..64 lanes owns a line's D, a wave owns
//            64 / WIDTH neighbouring lines and walks them forwards, then backwards.  The cost is
//            computed on the way from the two census words (__popcll) and never stored; the L of
//            the previous pixel stays in registers; its minimum over d is taken over the group's
//            lanes on DPP (group_min), d-1 / d+1 across the lanes' borders are one DPP wave shift
//            each.  Four u16 sums add as one 64-bit integer (S <= 2544 per field: no carry
//            crosses a field).  The horizontal launch's forward walk stores S, every other walk
//            adds to it; each lane only ever touches its own words, so there are no atomics and
//            the sum's order is fixed.  A walk is one dependent chain per wave, so the words of
//            the next kPathAhead pixels are loaded ahead of a pixel's recurrence, without
//            branches; 4 ahead is enough (8 measured the same: what is left is the instruction
//            count per pixel).  Along rows a wave's lines are 64 / WIDTH rows (one
//            S row of D * 2 bytes each per step); along columns they are neighbouring columns,
//            whose S rows are contiguous.
//   diagonals with n_paths = 8, twice more: the lines row = k + x, then the lines row = k - x, each
//            forwards and backwards with the same mechanics (comment at the kernel).  S <= 2544.
//   winner   a block per 1024-column segment of a row, a group per column: the first argmin of
//            S(y,x,.) with the parabola offset, and dR by an LDS minimum over the segment's
//            right-image pixels, so that S is read in rows here too (comment at the kernel).
//   check    one lane per pixel: rules 6 and 6b in place on disp16, rule 7.
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

// the words of pixel (y, x), both in range, for the lane whose 4 disparities start at d0 (its
// word gl_c of the pixel's dq words of S)
template <bool READ_S>
__device__ __forceinline__ PathStep path_load(const uint64_t* cenL, const uint64_t* cenR,
                                              const uint64_t* S, int y, int x, int cols, int d_min,
                                              int d0, int dq, int gl_c) {
    PathStep st;
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
    st.s = READ_S ? S[(size_t)(row + x) * dq + gl_c] : 0;
    return st;
}

// rule 3 for a lane's 4 disparities
__device__ __forceinline__ void path_costs(const PathStep& cur, int (&c)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = (cur.oob >> k) & 1 ? 63 : __popcll(cur.cl ^ cur.cr[k]);
}

// rule 4's recurrence: L of the previous pixel -> L of this one, kBig in a lane that is not `on`.
// A group whose lanes all hold kBig (m = kBig) gets L = c: the first pixel of a path.
template <int WIDTH>
__device__ __forceinline__ void path_recur(int (&L)[4], const int (&c)[4], int gl, int p1, int p2,
                                           bool on) {
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
    for (int k = 0; k < 4; k++) L[k] = on ? n[k] : kBig;
}

// a lane's 4 L as its word of S
__device__ __forceinline__ uint64_t path_pack(const int (&L)[4]) {
    return (uint64_t)(uint32_t)L[0] | ((uint64_t)(uint32_t)L[1] << 16) |
           ((uint64_t)(uint32_t)L[2] << 32) | ((uint64_t)(uint32_t)L[3] << 48);
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
        const int y = VERT ? p : line_c, x = VERT ? line_c : p;
        return path_load<decltype(read_s)::value>(cenL, cenR, S, y, x, cols, d_min, d0, dq, gl_c);
    };

    int L[4] = {kBig, kBig, kBig, kBig};
    // pixel p, the i-th of its walk, from its words
    auto step = [&](const PathStep& cur, int i, int p) {
        int c[4];
        path_costs(cur, c);
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) L[k] = act ? c[k] : kBig;
        } else {
            path_recur<WIDTH>(L, c, gl, p1, p2, act);
        }
        if (act) {
            const int y = VERT ? p : line, x = VERT ? line : p;
            // (cur.s = 0 on the storing walk)
            S[(size_t)((unsigned)y * cols + x) * dq + gl] = cur.s + path_pack(L);
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

// ------------------------------------------------------------------- diagonal paths ----
// Rule 4b.  One launch per family of lines: sy = +1 walks the lines row = k + x forwards (the path
// (+1, +1)) and backwards ((-1, -1)), sy = -1 the lines row = k - x ((-1, +1) and (+1, -1)).  The
// walk's mechanics are the path kernel's; a wave's 64 / WIDTH lines are neighbouring k, so at a
// column they are neighbouring rows, the access pattern of the walk along rows.  Every walk adds
// to S.
//   WRAP    k = 0 .. rows - 1, every line has all cols pixels, its row advancing by increment and
//           compare (the ring carries each pixel's row).
//   !WRAP   k = -(cols - 1) .. rows - 1 (sy = +1) or 0 .. rows + cols - 2 (sy = -1), rows + cols - 1
//           lines.  A wave walks the union of its lines' column spans; a lane whose pixel is
//           outside the image stores nothing and holds kBig, and path_recur turns a group of kBig
//           into L = c, so the pixel a line enters the image with is the first of its path
//           without a test of its own -- as is the first pixel of every walk.
struct DiagStep {
    PathStep w;
    int row;  // the pixel's row (!WRAP: as computed, in the image or not)
};

template <int WIDTH, bool WRAP>
__global__ __launch_bounds__(256) void stereo_diag_kernel(StereoArgs a, int sy) {
    constexpr int LPW = 64 / WIDTH;  // lines of a wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gl = lane & (WIDTH - 1);
    const int rows = a.rows, cols = a.cols, D = a.D;
    const int n_lines = WRAP ? rows : rows + cols - 1;
    const int line0 = (blockIdx.x * 4 + wave) * LPW;
    if (line0 >= n_lines) return;  // (wave-uniform; the kernel has no block barrier)
    const int line = line0 + lane / WIDTH;
    const int d0 = 4 * gl;
    const int dq = D >> 2, d_min = a.d_min, p1 = a.p1, p2 = a.p2;
    const bool act = line < n_lines && d0 < D;
    const int line_c = min(line, n_lines - 1), gl_c = min(gl, dq - 1);  // (as in the path kernel)
    const int kofs = !WRAP && sy > 0 ? -(cols - 1) : 0;
    const int k = line_c + kofs;  // the line's row at column 0
    // the columns at which one of the wave's lines ka .. kb is inside the image
    int x_lo = 0, x_hi = cols - 1;
    if (!WRAP) {
        const int ka = line0 + kofs, kb = min(line0 + LPW - 1, n_lines - 1) + kofs;
        x_lo = sy > 0 ? max(-kb, 0) : max(ka - rows + 1, 0);
        x_hi = sy > 0 ? min(rows - 1 - ka, cols - 1) : min(kb, cols - 1);
    }
    const int len = x_hi - x_lo + 1;  // >= 1: line ka has a pixel
    const size_t px = (size_t)rows * cols, pair = blockIdx.y;
    const uint64_t* cenL = a.census + pair * px;
    const uint64_t* cenR = a.census + ((size_t)a.n + pair) * px;
    uint64_t* S = (uint64_t*)(a.S + pair * px * D);

    int L[4];
    auto step = [&](const DiagStep& cur, int x) {
        int c[4];
        path_costs(cur.w, c);
        const bool on = act && (WRAP || (unsigned)cur.row < (unsigned)rows);
        path_recur<WIDTH>(L, c, gl, p1, p2, on);
        if (on) S[(size_t)((unsigned)cur.row * cols + x) * dq + gl] = cur.w.s + path_pack(L);
    };
    auto walk = [&](int dir) {
#pragma unroll
        for (int j = 0; j < 4; j++) L[j] = kBig;
        auto at = [&](int i) { return dir ? x_hi - min(i, len - 1) : x_lo + min(i, len - 1); };
        const int inc = dir ? -sy : sy;  // the row's step from a pixel of the walk to the next
        int r = 0;
        if (WRAP) {  // the first pixel's row, the one modulo of the walk
            r = (k + sy * at(0)) % rows;
            if (r < 0) r += rows;
        }
        // the loads of a walk are issued in the order of its pixels, so the running row is the
        // loaded pixel's; past the walk's end it runs on (in range) beside the last column
        auto load = [&](int x) {
            DiagStep st;
            if (WRAP) {
                st.row = r;
                r += inc;
                r = r == rows ? 0 : r;
                r = r < 0 ? rows - 1 : r;
            } else {
                st.row = k + sy * x;
            }
            const int y = WRAP ? st.row : min(max(st.row, 0), rows - 1);
            st.w = path_load<true>(cenL, cenR, S, y, x, cols, d_min, d0, dq, gl_c);
            return st;
        };
        DiagStep ring[kPathAhead];
#pragma unroll
        for (int j = 0; j < kPathAhead; j++) ring[j] = load(at(j));
        for (int i0 = 0; i0 < len; i0 += kPathAhead) {
#pragma unroll
            for (int j = 0; j < kPathAhead; j++) {
                const int i = i0 + j;
                if (i >= len) break;
                const DiagStep cur = ring[j];
                ring[j] = load(at(i + kPathAhead));
                step(cur, at(i));
            }
        }
    };
    walk(0);
    walk(1);
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
// UNIQ (rule 6b, uniq = the percentage): the group still holds the column's sums, so the smallest
// of those more than 1 away from d* is one more reduction; the verdict travels to the check as
// bit 8 of the d* word (d* <= 255).
template <int WIDTH, bool UNIQ>
__global__ __launch_bounds__(256) void stereo_winner_kernel(StereoArgs a, int kmin, int uniq) {
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
            uint64_t wk = ~(uint64_t)0;  // (UNIQ) the lane's sums, 0xffff where it has none
            if (act) {
                const uint64_t w = *(const uint64_t*)(Sp + (rowq + x) * D + d0);
                if (UNIQ) wk = w;
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
            int fail = 0;
            if (UNIQ) {  // rule 6b: some d with |d - d*| > 1 has S(d) (100 - uniq) < S(d*) 100
                int v2 = 0xffff;
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (abs(d0 + k - bd) > 1) v2 = min(v2, (int)(wk >> (16 * k)) & 0xffff);
#pragma unroll
                for (int o = 1; o < WIDTH; o <<= 1) v2 = min(v2, __shfl_xor(v2, o, 64));
                fail = v2 * (100 - uniq) < bv * 100 ? 0x100 : 0;
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
            a.dstar[pair * px + q] = (int16_t)(bd | fail);
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
    const int dw = a.dstar[o], ds = dw & 0xff;  // bit 8: rule 6b rejected the pixel
    const int xr = x - a.d_min - ds;
    bool valid = xr >= 0 && xr < cols && !(dw >> 8);
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
hipError_t launch_chunk_w(const StereoArgs& a, int n_paths, int uniq, hipStream_t st) {
    constexpr int LPB = 4 * (64 / WIDTH);  // lines of a path block
    const unsigned n = (unsigned)a.n;
    ERP_LAUNCH((stereo_path_kernel<WIDTH, false>), dim3((a.rows + LPB - 1) / LPB, n), dim3(256), 0,
               st, a);
    ERP_LAUNCH((stereo_path_kernel<WIDTH, true>), dim3((a.cols + LPB - 1) / LPB, n), dim3(256), 0,
               st, a);
    if (n_paths == 8)
        for (int sy = 1; sy >= -1; sy -= 2) {  // the two families of diagonal lines
            if (a.wrap)
                ERP_LAUNCH((stereo_diag_kernel<WIDTH, true>), dim3((a.rows + LPB - 1) / LPB, n),
                           dim3(256), 0, st, a, sy);
            else
                ERP_LAUNCH((stereo_diag_kernel<WIDTH, false>),
                           dim3((a.rows + a.cols - 1 + LPB - 1) / LPB, n), dim3(256), 0, st, a, sy);
        }
    // the winner's segments: every k whose kWinT columns or kWinT right-image pixels (those
    // start d_min + D - 1 to the left of the columns) meet the image
    const int off = a.d_min + a.D - 1;
    const int kmin = std::min(0, off >= 0 ? off / kWinT : -((-off + kWinT - 1) / kWinT));
    const int kmax = (a.cols + std::max(off, 0) + kWinT - 1) / kWinT;
    const dim3 grid((unsigned)(kmax - kmin), (unsigned)std::min(a.rows, 65535), n);
    if (uniq > 0)
        ERP_LAUNCH((stereo_winner_kernel<WIDTH, true>), grid, dim3(256), 0, st, a, kmin, uniq);
    else
        ERP_LAUNCH((stereo_winner_kernel<WIDTH, false>), grid, dim3(256), 0, st, a, kmin, 0);
    return hipGetLastError();
}

// one chunk: census, the two path launches (and the two diagonal ones), the winner and the check
hipError_t launch_chunk(const StereoArgs& a, int n_paths, int uniq, hipStream_t st) {
    const unsigned n = (unsigned)a.n;
    const size_t px = (size_t)a.rows * a.cols;
    const size_t tiles = (size_t)((a.cols + kCenTW - 1) / kCenTW) * ((a.rows + kCenTH - 1) / kCenTH);
    ERP_LAUNCH(stereo_census_kernel, dim3((unsigned)tiles, 2 * n), dim3(256), 0, st, a);
    const int w = a.D / 4;  // lanes a line's D needs; the group is the power of two above
    hipError_t e;
    if (w <= 4)
        e = launch_chunk_w<4>(a, n_paths, uniq, st);
    else if (w <= 8)
        e = launch_chunk_w<8>(a, n_paths, uniq, st);
    else if (w <= 16)
        e = launch_chunk_w<16>(a, n_paths, uniq, st);
    else if (w <= 32)
        e = launch_chunk_w<32>(a, n_paths, uniq, st);
    else
        e = launch_chunk_w<64>(a, n_paths, uniq, st);
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

void erp_stereo_params_ex_default(erp_stereo_params_ex* p) {
    if (!p) return;
    erp_stereo_params_default(&p->base);
    p->n_paths = 4;
    p->uniqueness = 0;
    p->reserved[0] = p->reserved[1] = 0;
}

erp_status erp_stereo_rows_ex_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                                  int32_t n_pairs, int32_t rows, int32_t cols,
                                  const erp_stereo_params_ex* params_ex, int16_t* d_disp16,
                                  float* d_depth, void* stream) {
    if (!ctx || !params_ex || n_pairs < 0 || rows < 1 || cols < 1 ||
        (int64_t)rows * cols > erp::kMaxPixels || !erp::params_ok(params_ex->base))
        return ERP_INVALID_ARG;
    const int n_paths = params_ex->n_paths, uniq = params_ex->uniqueness;
    if ((n_paths != 4 && n_paths != 8) || uniq < 0 || uniq > 99 || params_ex->reserved[0] ||
        params_ex->reserved[1])
        return ERP_INVALID_ARG;
    const erp_stereo_params* params = &params_ex->base;
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
        if (erp::launch_chunk(a, n_paths, uniq, st) != hipSuccess) return ERP_HIP_ERROR;
    }
    return ERP_OK;
}

// the same implementation with n_paths = 4, uniqueness = 0
erp_status erp_stereo_rows_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                               int32_t n_pairs, int32_t rows, int32_t cols,
                               const erp_stereo_params* params, int16_t* d_disp16,
                               float* d_depth, void* stream) {
    if (!params) return ERP_INVALID_ARG;
    erp_stereo_params_ex ex;
    erp_stereo_params_ex_default(&ex);
    ex.base = *params;
    return erp_stereo_rows_ex_dev(ctx, d_left, d_right, n_pairs, rows, cols, &ex, d_disp16, d_depth,
                                  stream);
}

}  // extern "C"

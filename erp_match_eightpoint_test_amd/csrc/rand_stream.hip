// rand_stream.hip -- the rand stream: glibc rand() state that continues from one call to the
// next, as the reference's process-global rand() does (every eight_point::find of a process
// goes on where the previous one stopped: one_image_test/main.cpp:135-137).
//
// The state (31-word window, seed, draws consumed) lives in device memory.  A consuming launch
// hands every pair of the launch its own start window and advances the state, without a host
// round trip: pair p starts e_p = sum_{q<p} d_q draws past the state, d_q = iters (M_q - 1) for
// a pair the sampler runs and 0 otherwise, and M_q is only known on the device.  The jump is
// x^e mod P(x) = x^31 - x^28 - 1 over Z/2^32 (erp_jump_poly.hpp) as a product of table powers,
// one per non-zero byte of e (x^(k 256^j), k < 256, j < 8), for any 64-bit e.
//
// The same polynomial arithmetic on the host (glibc_poly_*) positions a stream that no GPU call
// has used yet, and replaces the O(offset) loop of host_glibc_window for large offsets.
//
// The stream's host side is at the end of the file: the state's way to the device and back,
// the process streams and the erp_rand_stream_* entry points of include/erp_match.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/erp_match.h"
#include "erp_ctx.hpp"
#include "erp_jump_poly.hpp"
#include "erp_kernels.hpp"
#include "erp_launch.hpp"

namespace erp {

// ================================================================ host ==================
namespace {

// out = a * b mod P (x^d = x^(d-3) + x^(d-31) folds the product's top); out may alias a or b
void poly_mul(const uint32_t a[31], const uint32_t b[31], uint32_t out[31]) {
    uint32_t c[61] = {};
    for (int i = 0; i < 31; i++)
        for (int j = 0; j < 31; j++) c[i + j] += a[i] * b[j];
    for (int d = 60; d >= 31; d--) {
        c[d - 3] += c[d];
        c[d - 31] += c[d];
    }
    for (int k = 0; k < 31; k++) out[k] = c[k];
}

}  // namespace

void glibc_poly_pow(uint64_t e, uint32_t out[31]) {
    uint32_t sq[31] = {}, acc[31] = {};
    sq[1] = 1;   // x
    acc[0] = 1;  // 1
    for (; e; e >>= 1) {
        if (e & 1) poly_mul(acc, sq, acc);
        if (e >> 1) poly_mul(sq, sq, sq);
    }
    memcpy(out, acc, sizeof(acc));
}

void glibc_poly_apply(const uint32_t c[31], uint32_t win[31]) {
    uint32_t ext[61];
    for (int k = 0; k < 31; k++) ext[k] = win[k];
    for (int d = 31; d < 61; d++) ext[d] = ext[d - 3] + ext[d - 31];
    for (int t = 0; t < 31; t++) {
        uint32_t acc = 0;
        for (int j = 0; j < 31; j++) acc += c[j] * ext[t + j];
        win[t] = acc;
    }
}

void glibc_window_jump(uint32_t win[31], uint64_t n) {
    if (n == 0) return;
    uint32_t c[31];
    glibc_poly_pow(n, c);
    glibc_poly_apply(c, win);
}

void glibc_window_seq(uint32_t seed, uint64_t offset, uint32_t out[31]) {
    int32_t r0[34];
    if (seed == 0) seed = 1;
    r0[0] = (int32_t)seed;
    for (int i = 1; i < 31; i++) {
        const long hi = r0[i - 1] / 127773, lo = r0[i - 1] % 127773;
        long word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r0[i] = (int32_t)word;
    }
    for (int i = 31; i < 34; i++) r0[i] = r0[i - 31];
    uint32_t ring[34];
    for (int i = 0; i < 34; i++) ring[i] = (uint32_t)r0[i];
    uint64_t pos = 34;                    // absolute index of the next word
    const uint64_t end = 344 + offset;    // draw k uses word k + 344
    for (; pos < end; pos++) {
        const uint32_t s = (uint32_t)(pos % 34);
        ring[s] = ring[(pos - 3) % 34] + ring[(pos - 31) % 34];
    }
    for (int j = 0; j < 31; j++) out[j] = ring[(end - 31 + j) % 34];
}

// ============================================================== device ==================
namespace {

// x^(31+d) mod P, d = 0..29 (kernels.hip keeps its own copy: constant memory is per
// translation unit)
__constant__ uint32_t s_red[30][31];

// The power table, in device memory (one per device, stream_table()): entry (j, k) = x^(k 256^j)
// mod P, j < 8, k < 256, kTabRow words each.  A 64-bit exponent is then at most 8 factors -- 4
// dependent products at the headline's e ~ 2^32 where the bit-wise table of jump_prep_kernel
// (x^(2^b)) would need popcount(e) - 1 ~ 15; this chain is the whole latency of the kernels.
constexpr int kTabRow = 32;
constexpr size_t kTabWords = (size_t)8 * 256 * kTabRow;

// LDS of one wave's jump: the table factors of the exponent's non-zero bytes, staged once with
// all loads in flight (pmul_wave reads its second operand per lane: straight from memory that
// is a dependent load per term, kernels.hip jump_prep_kernel), two product buffers, the window
// extended to 61 words
struct JumpLds {
    uint32_t fac[8][32];
    uint32_t tq[2][32];
    uint32_t ext[64];
};

// One wave (a block of 64 threads): x^e mod P -> L.tq[returned index].  (non-zero bytes of
// e) - 1 dependent products.
__device__ int poly_pow_wave(uint64_t e, const uint32_t* __restrict__ tab, JumpLds& L,
                             const uint32_t (&cred)[30]) {
    const int lane = threadIdx.x;
    int nf = 0;
    for (int j = 0; j < 8; j++) {  // (uniform)
        const uint32_t k = (uint32_t)(e >> (8 * j)) & 255u;
        if (!k) continue;
        if (lane < 31) L.fac[nf][lane] = tab[((size_t)j * 256 + k) * kTabRow + lane];
        nf++;
    }
    if (lane < 31) L.tq[0][lane] = nf ? L.fac[0][lane] : (lane == 0 ? 1u : 0u);
    __syncthreads();
    int cur = 0;
    for (int f = 1; f < nf; f++) {
        pmul_wave(L.tq[cur], L.fac[f], L.tq[cur ^ 1], cred);
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// One wave: the window in L.ext[0..30] moved on by the polynomial c (LDS); lanes t < 31
// return word t of the new window (apply_coop's form, kernels.hip).
__device__ uint32_t apply_wave(const uint32_t* c, JumpLds& L) {
    const int lane = threadIdx.x;
    if (lane == 0) {
        uint32_t t[61];
#pragma unroll
        for (int k = 0; k < 31; k++) t[k] = L.ext[k];
#pragma unroll
        for (int d = 31; d < 61; d++) {
            t[d] = t[d - 3] + t[d - 31];
            L.ext[d] = t[d];
        }
    }
    __syncthreads();
    uint32_t acc = 0;
    if (lane < 31) {
#pragma unroll
        for (int j = 0; j < 31; j++) acc += c[j] * L.ext[lane + j];
    }
    __syncthreads();
    return acc;
}

__device__ __forceinline__ void load_cred(uint32_t (&cred)[30]) {
#pragma unroll
    for (int d = 0; d < 30; d++) cred[d] = threadIdx.x < 31 ? s_red[d][threadIdx.x] : 0u;
}

// draws of pair q: the sampler's own skip condition (kernels.hip jump_prep_kernel,
// sampler_window_kernel) decides whether the pair consumes
__device__ __forceinline__ uint64_t pair_draws(int M, int iters, double sample_frac) {
    return ((int)(M * sample_frac) < 1 || M < 2) ? 0ull : (uint64_t)iters * (uint64_t)(M - 1);
}

// Block p < n_pairs (one wave): pair p's start window; block n_pairs: the stream's next state.
// Each block forms its own exclusive prefix e_p of the pairs' draws (lane-strided 64-bit sums
// over q < p, then a wave reduction): ceil(p / 64) loads per lane instead of a scan launch of
// its own in front of a kernel that is a handful of dependent products long.
// The state's window is only read here; stream_commit_kernel moves the next state in after
// every block of this launch has finished.
__global__ __launch_bounds__(64) void stream_assign_kernel(const int32_t* __restrict__ counts,
                                                           int n_pairs, int iters,
                                                           double sample_frac,
                                                           const uint32_t* __restrict__ tab,
                                                           uint32_t* __restrict__ state,
                                                           uint32_t* __restrict__ w0s) {
    __shared__ JumpLds L;
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p < n_pairs && pair_draws(counts[p], iters, sample_frac) == 0) return;  // (uniform)
    uint64_t e = 0;
    for (int q = lane; q < p; q += 64) e += pair_draws(counts[q], iters, sample_frac);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) e += __shfl_xor((unsigned long long)e, o, 64);
    uint32_t cred[30];
    load_cred(cred);
    if (lane < 31) L.ext[lane] = state[kStreamWin + lane];
    const int cur = poly_pow_wave(e, tab, L, cred);
    const uint32_t w = apply_wave(L.tq[cur], L);
    if (p < n_pairs) {
        if (lane < 31) w0s[(size_t)p * 31 + lane] = w;
    } else {
        if (lane < 31) state[kStreamNextWin + lane] = w;
        if (lane == 0) {
            const uint64_t draws = *reinterpret_cast<const uint64_t*>(state + kStreamDraws);
            *reinterpret_cast<uint64_t*>(state + kStreamNextDraws) = draws + e;  // wraps mod 2^64
        }
    }
}

__global__ __launch_bounds__(64) void stream_commit_kernel(uint32_t* __restrict__ state) {
    const int lane = threadIdx.x;
    if (lane < 31) state[kStreamWin + lane] = state[kStreamNextWin + lane];
    if (lane == 0)
        *reinterpret_cast<uint64_t*>(state + kStreamDraws) =
            *reinterpret_cast<const uint64_t*>(state + kStreamNextDraws);
}

// erp_rand_stream_set / _advance on a stream whose state is on the device (one wave)
__global__ __launch_bounds__(64) void stream_jump_kernel(const uint32_t* __restrict__ tab,
                                                         uint32_t* __restrict__ state, int set,
                                                         uint32_t seed, uint64_t n) {
    __shared__ JumpLds L;
    const int lane = threadIdx.x;
    uint32_t cred[30];
    load_cred(cred);
    if (set) {
        // srandom(seed) and glibc's 310 discarded words: the window before draw 0
        // (glibc_window_seq with offset 0)
        if (lane == 0) {
            uint32_t* ring = &L.fac[0][0];  // 34 words (the factors are staged after this)
            int32_t r = (int32_t)(seed ? seed : 1u);
            ring[0] = (uint32_t)r;
            for (int i = 1; i < 31; i++) {
                const long hi = r / 127773, lo = r % 127773;
                long word = 16807 * lo - 2836 * hi;
                if (word < 0) word += 2147483647;
                r = (int32_t)word;
                ring[i] = (uint32_t)r;
            }
            for (int i = 31; i < 34; i++) ring[i] = ring[i - 31];
            for (int pos = 34; pos < 344; pos++)
                ring[pos % 34] = ring[(pos - 3) % 34] + ring[(pos - 31) % 34];
            for (int j = 0; j < 31; j++) L.ext[j] = ring[(344 - 31 + j) % 34];
        }
    } else if (lane < 31) {
        L.ext[lane] = state[kStreamWin + lane];
    }
    __syncthreads();
    const int cur = poly_pow_wave(n, tab, L, cred);
    const uint32_t w = apply_wave(L.tq[cur], L);
    if (lane < 31) state[kStreamWin + lane] = w;
    if (lane == 0) {
        uint64_t* draws = reinterpret_cast<uint64_t*>(state + kStreamDraws);
        if (set) {
            state[kStreamSeed] = seed ? seed : 1u;
            *draws = n;
        } else {
            *draws += n;
        }
    }
}

// the power table of the current device (built and uploaded on first use, never freed)
std::mutex g_tab_mu;
std::vector<uint32_t*> g_tab;  // by device

const uint32_t* stream_table() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
    std::lock_guard<std::mutex> g(g_tab_mu);
    if (g_tab.size() <= (size_t)dev) g_tab.resize((size_t)dev + 1, nullptr);
    if (g_tab[dev]) return g_tab[dev];
    std::vector<uint32_t> h(kTabWords, 0u);
    uint32_t base[31] = {};
    base[1] = 1;  // x^(256^0)
    for (int j = 0; j < 8; j++) {
        uint32_t* row = &h[(size_t)j * 256 * kTabRow];
        row[0] = 1;  // k = 0: the polynomial 1 (never staged)
        memcpy(row + kTabRow, base, sizeof(base));
        for (int k = 2; k < 256; k++)
            poly_mul(row + (size_t)(k - 1) * kTabRow, base, row + (size_t)k * kTabRow);
        uint32_t next[31];
        poly_mul(row + (size_t)255 * kTabRow, base, next);  // x^(256^(j+1))
        memcpy(base, next, sizeof(base));
    }
    uint32_t* d = nullptr;
    if (hipMalloc(&d, kTabWords * 4) != hipSuccess) return nullptr;
    if (hipMemcpy(d, h.data(), kTabWords * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return nullptr;
    }
    g_tab[dev] = d;
    return d;
}

}  // namespace

void init_stream_constants() {
    uint32_t red[30][31];
    uint32_t x[31] = {};
    x[1] = 1;
    glibc_poly_pow(31, red[0]);
    for (int d = 1; d < 30; d++) poly_mul(red[d - 1], x, red[d]);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(s_red), red, sizeof(red));
}

bool stream_tables_ready() { return stream_table() != nullptr; }

hipError_t launch_stream_assign(const int32_t* counts, int n_pairs, int iters, double sample_frac,
                                uint32_t* state, uint32_t* w0s, hipStream_t st) {
    if (n_pairs < 1 || iters < 1) return hipErrorInvalidValue;
    const uint32_t* tab = stream_table();
    if (!tab) return hipErrorOutOfMemory;
    ERP_LAUNCH(stream_assign_kernel, dim3(n_pairs + 1), dim3(64), 0, st, counts, n_pairs, iters,
               sample_frac, tab, state, w0s);
    ERP_LAUNCH(stream_commit_kernel, dim3(1), dim3(64), 0, st, state);
    return hipGetLastError();
}

hipError_t launch_stream_jump(uint32_t* state, int set, uint32_t seed, uint64_t n,
                              hipStream_t st) {
    const uint32_t* tab = stream_table();
    if (!tab) return hipErrorOutOfMemory;
    ERP_LAUNCH(stream_jump_kernel, dim3(1), dim3(64), 0, st, tab, state, set, seed, n);
    return hipGetLastError();
}

erp_status rs_to_device(erp_rand_stream* s, int device) {
    std::lock_guard<std::mutex> g(s->mu);
    if (s->d_state) return s->device == device ? ERP_OK : ERP_INVALID_ARG;
    if (s->device >= 0 && s->device != device) return ERP_INVALID_ARG;  // a process stream
    uint32_t h[kStreamStateWords] = {};
    memcpy(h + kStreamWin, s->win, sizeof(s->win));
    h[kStreamSeed] = s->seed;
    memcpy(h + kStreamDraws, &s->draws, 8);
    uint32_t* d = nullptr;
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return ERP_OUT_OF_MEMORY;
    hipEvent_t ev = nullptr;
    if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(d);
        return ERP_HIP_ERROR;
    }
    s->d_state = d;
    s->ev = ev;
    s->device = device;
    return ERP_OK;
}

}  // namespace erp

// ================================================= the stream's host side ===============
// Small offsets step the recurrence; above kSeqOffsets the window before draw 0 is moved on by
// x^offset mod P (glibc_poly_pow: ~128 products of 31 x 31 words whatever the offset).
constexpr uint64_t kSeqOffsets = 4096;
void host_glibc_window(uint32_t seed, uint64_t offset, uint32_t out[31]) {
    if (offset <= kSeqOffsets) return erp::glibc_window_seq(seed, offset, out);
    erp::glibc_window_seq(seed, 0, out);
    erp::glibc_window_jump(out, offset);
}

namespace {

// the stream's (seed, draws, window) on the host, after its last device update; s->mu held
erp_status rs_fetch(erp_rand_stream* s) {
    if (!s->d_state) return ERP_OK;
    ERP_CK(hipSetDevice(s->device));
    if (s->pending) ERP_CK(hipEventSynchronize(s->ev));
    uint32_t h[erp::kStreamNextWin];
    ERP_CK(hipMemcpy(h, s->d_state, sizeof(h), hipMemcpyDeviceToHost));
    memcpy(s->win, h + erp::kStreamWin, sizeof(s->win));
    s->seed = h[erp::kStreamSeed];
    memcpy(&s->draws, h + erp::kStreamDraws, 8);
    return ERP_OK;
}

// set (seed, offset) or advance by n; s->mu held.  Host arithmetic before the first device use,
// one wave on the device after it (ordered by the stream's event, on the null stream)
erp_status rs_jump(erp_rand_stream* s, bool set, uint32_t seed, uint64_t n) {
    if (set && seed == 0) seed = 1;
    if (!s->d_state) {
        if (set) {
            host_glibc_window(seed, n, s->win);
            s->seed = seed;
            s->draws = n;
        } else {
            erp::glibc_window_jump(s->win, n);
            s->draws += n;
        }
        return ERP_OK;
    }
    ERP_CK(hipSetDevice(s->device));
    if (s->pending) ERP_CK(hipStreamWaitEvent(nullptr, s->ev, 0));
    ERP_CK(erp::launch_stream_jump(s->d_state, set ? 1 : 0, seed, n, nullptr));
    ERP_CK(hipEventRecord(s->ev, nullptr));
    s->pending = true;
    return ERP_OK;
}

std::mutex g_process_mu;
std::vector<erp_rand_stream*> g_process_streams;  // by device, never freed

}  // namespace

extern "C" {

erp_status erp_rand_stream_create(uint32_t seed, uint64_t offset, erp_rand_stream** out) {
    if (!out) return ERP_INVALID_ARG;
    erp_rand_stream* s = new (std::nothrow) erp_rand_stream();
    if (!s) return ERP_OUT_OF_MEMORY;
    (void)rs_jump(s, true, seed, offset);
    *out = s;
    return ERP_OK;
}

erp_status erp_rand_stream_destroy(erp_rand_stream* s) {
    if (!s || s->process_owned) return ERP_INVALID_ARG;
    if (s->d_state) {
        (void)hipSetDevice(s->device);
        if (s->pending) (void)hipEventSynchronize(s->ev);
        (void)hipEventDestroy(s->ev);
        (void)hipFree(s->d_state);
    }
    delete s;
    return ERP_OK;
}

erp_status erp_rand_stream_get(erp_rand_stream* s, uint32_t* seed, uint64_t* draws) {
    if (!s) return ERP_INVALID_ARG;
    std::lock_guard<std::mutex> g(s->mu);
    const erp_status es = rs_fetch(s);
    if (es != ERP_OK) return es;
    if (seed) *seed = s->seed;
    if (draws) *draws = s->draws;
    return ERP_OK;
}

erp_status erp_rand_stream_set(erp_rand_stream* s, uint32_t seed, uint64_t offset) {
    if (!s) return ERP_INVALID_ARG;
    std::lock_guard<std::mutex> g(s->mu);
    return rs_jump(s, true, seed, offset);
}

erp_status erp_rand_stream_advance(erp_rand_stream* s, uint64_t n) {
    if (!s) return ERP_INVALID_ARG;
    std::lock_guard<std::mutex> g(s->mu);
    return rs_jump(s, false, 0, n);
}

erp_status erp_rand_stream_process(int32_t device, erp_rand_stream** out) {
    if (!out || device < 0 || device >= 1024) return ERP_INVALID_ARG;
    std::lock_guard<std::mutex> g(g_process_mu);
    if (g_process_streams.size() <= (size_t)device) g_process_streams.resize((size_t)device + 1);
    erp_rand_stream*& s = g_process_streams[(size_t)device];
    if (!s) {
        s = new (std::nothrow) erp_rand_stream();
        if (!s) return ERP_OUT_OF_MEMORY;
        (void)rs_jump(s, true, 1, 0);
        s->device = device;
        s->process_owned = true;
    }
    *out = s;
    return ERP_OK;
}

erp_status erp_rand_stream_shuffle_prefix(erp_rand_stream* s, int32_t m, int32_t n,
                                          int32_t* h_idx) {
    if (!s || m < 1 || n < 0 || n > m || (n > 0 && !h_idx)) return ERP_INVALID_ARG;
    std::lock_guard<std::mutex> g(s->mu);
    const erp_status es = rs_fetch(s);
    if (es != ERP_OK) return es;
    erp_shuffle_prefix_window(s->win, m, n, h_idx);  // (steps the window m - 1 draws)
    s->draws += (uint64_t)(m - 1);
    if (s->d_state) {  // (rs_fetch waited for the last device update; the lock keeps others out)
        uint32_t h[erp::kStreamNextWin];
        memcpy(h + erp::kStreamWin, s->win, sizeof(s->win));
        h[erp::kStreamSeed] = s->seed;
        memcpy(h + erp::kStreamDraws, &s->draws, 8);
        ERP_CK(hipMemcpy(s->d_state, h, sizeof(h), hipMemcpyHostToDevice));
        s->pending = false;
    }
    return ERP_OK;
}

}  // extern "C"

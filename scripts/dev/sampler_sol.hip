// Speed-of-light probe for the glibc-replay sampler (VERDICT r05 "next" 1).
//
// The same per-lane backwards ring (r[n-31] = r[n] - r[n-3], the glibc TYPE_3 recurrence run in
// reverse), the same Granlund-Montgomery magic quotient + v_mad_i32_i24 remainder, the same launch
// shape as sampler_kernel<0> (one 64-lane wave per 64 iterations, grid (waves, pairs), the pair's
// draws i = M-1 .. 1 in blocks of 31 with the block's divisor constants by scalar loads) -- with
// the bookkeeping cut away stage by stage:
//   V0  generator only:                 ring subtract, >> 1, xor into an accumulator
//   V1  generator + modulo (the floor):  + mulhi, shift, mad_i24 remainder
//   V2  + the i >= s bookkeeping on every step: clamp, LDS masked OR with return, bit extract
//       and placement, one coalesced selection-word store per block (no prefix / mixed blocks)
//   V3  V2 with the magic shift as a compile-time constant per power-of-two range of d
//   V4  V3 with the selection bit accumulated through the carry (v_and + v_add_co + v_addc)
//   V5 - V7  the position-major bitmap and the whole replay in both layouts (further down)
//   V10 V9, byte for byte, launched with a larger dynamic LDS allocation than it uses (the
//       library's bound-sized one): what the allocation alone costs in occupancy
// The real kernel (prefix and mixed blocks included) is timed beside it by sampler_sol.py through
// the library's own stage timer.  Results are not the sampler's (the windows are random words):
// this measures instruction cost, not parity.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC scripts/dev/sampler_sol.hip \
//         -o devlibs/libsampler_sol.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

namespace {

typedef __attribute__((address_space(3))) uint32_t lds_u32;

__device__ __forceinline__ uint32_t mskor_rtn(uint32_t addr, uint32_t mask, uint32_t data) {
    uint32_t old;
    asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3" : "=v"(old) : "v"(addr), "v"(mask), "v"(data)
                 : "memory");
    return old;
}
__device__ __forceinline__ void wait_lag(uint32_t& o, int v) {
    if (30 - v >= 8) asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(o) : : "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o) : : "memory");
}
__device__ __forceinline__ uint32_t mad24(uint32_t q, int negd, uint32_t x) {
    int j;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(j) : "v"(q), "s"(negd), "v"(x));
    return (uint32_t)j;
}

constexpr int kLag = 8;

// one block of 31 steps i0 .. i0-30 (all >= 1 when FULL); SH >= 0: the magic shift as a constant
template <int V, int SH, bool I24>
__device__ __forceinline__ uint32_t sol_block(uint32_t (&ring)[31], uint32_t bm_lane, int i0, int s,
                                              const uint64_t* __restrict__ mtab, uint32_t& acc) {
    uint64_t mt[31];
#pragma unroll
    for (int u = 0; u < 31; u++) mt[u] = mtab[i0 - u + 1];
    uint32_t olds[31], pos[31], bits[31];
    uint32_t nw = 0;
#pragma unroll
    for (int u = 0; u < 31 + kLag; u++) {
        if (u < 31) {
            const int d = i0 - u + 1;
            const int slot = 30 - u;
            const uint32_t rv = ring[slot];
            ring[slot] = rv - ring[(slot + 28) % 31];
            const uint32_t x = rv >> 1;
            if (V == 0) { acc ^= x; continue; }
            const uint32_t hi = __umulhi(x, (uint32_t)mt[u]);
            const uint32_t q = SH >= 0 ? hi >> SH : hi >> (uint32_t)(mt[u] >> 32);
            uint32_t j = I24 ? mad24(q, -d, x) : x - q * (uint32_t)d;
            if (V == 1) { acc ^= j; continue; }
            j = min(j, (uint32_t)s);
            uint32_t a;
            asm("v_lshl_add_u32 %0, %1, 8, %2" : "=v"(a) : "v"(j >> 5), "v"(bm_lane));
            bits[u] = 1u << (j & 31);
            olds[u] = mskor_rtn(a, bits[u], 0u);
            pos[u] = j;
        }
        const int v = u - kLag;
        if (V >= 2 && v >= 0) {
            wait_lag(olds[v], v);
            if (V == 4) {
                // carry = (old & bit) != 0, shifted in from the bottom (bit order reversed)
                const uint32_t t = olds[v] & bits[v];
                uint32_t c;
                asm volatile("v_add_co_u32 %0, vcc, -1, %1\n\tv_addc_co_u32 %2, vcc, %2, %2, vcc"
                             : "=&v"(c), "+v"(nw) : "v"(t) : "vcc");
                (void)c;
            } else {
                nw |= __builtin_amdgcn_ubfe(olds[v], pos[v], 1) << v;
            }
        }
    }
    return V == 4 ? __builtin_bitreverse32(nw) >> 1 : nw;
}

template <int V>
__global__ __launch_bounds__(64) void sol_kernel(const int32_t* __restrict__ counts, int nwaves,
                                                 double frac, const uint64_t* __restrict__ mtab,
                                                 uint32_t* __restrict__ out, int nbw, int nalloc) {
    extern __shared__ uint32_t bm[];
    const int p = blockIdx.y, w = blockIdx.x, lane = threadIdx.x;
    const int M = counts[p];
    const int s = (int)(M * frac);
    if (V >= 2)
        for (int k = 0; k < nalloc; k++)
            bm[k * 64 + lane] = k < (s >> 5) ? ~0u : k == (s >> 5) ? (1u << (s & 31)) - 1u : 0u;
    uint32_t ring[31];
    uint32_t h = (uint32_t)(p * 7919 + w * 104729 + lane * 31337) | 1u;
#pragma unroll
    for (int t = 0; t < 31; t++) {
        h ^= h << 13; h ^= h >> 17; h ^= h << 5;
        ring[t] = h;
    }
    const uint32_t bm_lane = (uint32_t)(size_t)(lds_u32*)bm + 4u * (uint32_t)lane;
    uint32_t* o = out + ((size_t)p * nwaves + w) * (size_t)nbw * 64 + lane;
    uint32_t acc = 0;
    int i = M - 1, b = 0;
    while (i - 30 >= 1) {
        uint32_t word;
        if (V == 3 || V == 4) {
            // the shift is constant when the block's 31 divisors share ceil(log2 d)
            // ceil(log2 d) = bit length of d - 1: d = i + 1 .. i - 29
            const int lhi = 32 - __builtin_clz((uint32_t)i);
            const int llo = 32 - __builtin_clz((uint32_t)(i - 30));
            const int l = lhi == llo ? lhi : -1;
            switch (l) {
#define SOL_CASE(L) case L: word = sol_block<V, L - 1, true>(ring, bm_lane, i, s, mtab, acc); break;
                SOL_CASE(9) SOL_CASE(10) SOL_CASE(11) SOL_CASE(12) SOL_CASE(13)
#undef SOL_CASE
                default: word = i - 30 >= 256 ? sol_block<V, -1, true>(ring, bm_lane, i, s, mtab, acc)
                                              : sol_block<V, -1, false>(ring, bm_lane, i, s, mtab, acc);
                         break;
            }
        } else {
            word = i - 30 >= 256 ? sol_block<V, -1, true>(ring, bm_lane, i, s, mtab, acc)
                                 : sol_block<V, -1, false>(ring, bm_lane, i, s, mtab, acc);
        }
        if (V >= 2) o[(size_t)b * 64] = word;
        i -= 31;
        b++;
    }
    o[(size_t)b * 64] = acc ^ (uint32_t)i;
}

// ---- position-major bitmap (V5 / V6) and the lane-major full replay (V7) ---------------------
// V5 / V6 turn the bitmap round: one word per position, one bit per lane -- words
// [half][position] (half = lane >> 5; [position][half] would put a half-wave's 32 lanes on the
// 16 even banks only).  A lane's bit mask and bit index are constants in registers and the
// address is one v_lshl_add_u32 of j:
//   V5  V2's all-draw blocks in that form: clamp, address, ds_and_rtn_b32(~lanebit), bit extract
//       and placement (9 VALU per draw against 11)
//   V6  V5 plus the prefix blocks (bm[i] one broadcast read at a wave-uniform address, the copied
//       bit rd & lanebit, one masked OR) and the straddling / ending blocks, i.e. the whole replay
//   V7  the whole replay on the lane-major bitmap (the shipped kernel's blocks restated): V6's
//       stand-in for sampler_kernel<0> inside the probe
//   V8 / V9  V5 / V6 with the draws clamped to position s + (lane & 31) instead of s: most draws
//       of a replay have j >= s (i runs from M - 1 down to s = M / 4), and clamped to ONE word
//       they make every wave-op a 32-lane same-address atomic per half, which the LDS serialises;
//       per-lane clamp words (all clear, 32 more positions allocated per half) put the clamped
//       lanes on 32 distinct banks
struct PmLane {
    uint32_t base;  // LDS byte address of the half's position 0
    uint32_t bit;   // 1 << (lane & 31)
    uint32_t nbit;  // ~bit
    uint32_t idx;   // lane & 31
    uint32_t cap;   // the draws' clamp: s, or s + idx (V8 / V9)
};
__device__ __forceinline__ uint32_t and_rtn(uint32_t addr, uint32_t data) {
    uint32_t old;
    asm volatile("ds_and_rtn_b32 %0, %1, %2" : "=v"(old) : "v"(addr), "v"(data) : "memory");
    return old;
}
__device__ __forceinline__ uint32_t pos_addr(uint32_t base, uint32_t j) {
    uint32_t a;
    asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(a) : "v"(j), "v"(base));
    return a;
}
__device__ __forceinline__ uint32_t sol_mod(bool i24, uint32_t x, uint64_t mt, int d) {
    const uint32_t q = __umulhi(x, (uint32_t)mt) >> (uint32_t)(mt >> 32);
    return i24 ? mad24(q, -d, x) : x - q * (uint32_t)d;
}
// ds_read_b32 at a constant byte offset from a (no address arithmetic per step)
template <int OFF>
__device__ __forceinline__ uint32_t read_off(uint32_t a, bool clobber) {
    uint32_t rd;
    if (clobber) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(rd) : "v"(a), "n"(OFF) : "memory");
    else asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(rd) : "v"(a), "n"(OFF));
    return rd;
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a
// constant expression in the body (the reads' immediate offsets)
template <typename F, int... U>
__device__ __forceinline__ void static_for(std::integer_sequence<int, U...>, F&& f) {
    (f(std::integral_constant<int, U>{}), ...);
}

template <bool I24>
__device__ __forceinline__ uint32_t pm_draws(uint32_t (&ring)[31], const PmLane& pl, int i0, int s,
                                             const uint64_t* __restrict__ mtab) {
    uint64_t mt[31];
#pragma unroll
    for (int u = 0; u < 31; u++) mt[u] = mtab[i0 - u + 1];
    uint32_t olds[31];
    uint32_t nw = 0;
#pragma unroll
    for (int u = 0; u < 31 + kLag; u++) {
        if (u < 31) {
            const int slot = 30 - u;
            const uint32_t rv = ring[slot];
            ring[slot] = rv - ring[(slot + 28) % 31];
            const uint32_t j = min(sol_mod(I24, rv >> 1, mt[u], i0 - u + 1), pl.cap);
            olds[u] = and_rtn(pos_addr(pl.base, j), pl.nbit);
        }
        const int v = u - kLag;
        if (v >= 0) {
            wait_lag(olds[v], v);
            nw |= __builtin_amdgcn_ubfe(olds[v], pl.idx, 1) << v;
        }
    }
    return nw;
}

// steps 1 <= i < s: bm[i] read back per step (after the previous step's masked OR: a wave's LDS
// ops complete in order); POS: position-major, else lane-major [word][lane]
template <bool POS, bool I24>
__device__ __forceinline__ uint32_t sol_prefix(uint32_t (&ring)[31], const PmLane& pl,
                                               uint32_t bm_lane, int i0,
                                               const uint64_t* __restrict__ mtab) {
    uint64_t mt[31];
    uint32_t nw = 0, prev = 0, ppos = 0;
    const uint32_t rbase = pl.base + 4u * (uint32_t)(i0 - 30);
    static_for(std::make_integer_sequence<int, 31>{}, [&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
        const int ii = i0 - u;
        if (u == 0 || u == 16)
#pragma unroll
            for (int k = u; k < (u == 0 ? 16 : 31); k++) mt[k] = mtab[i0 - k + 1];
        uint32_t rd;
        if (POS) {
            rd = read_off<4 * (30 - u)>(rbase, u == 0 || u == 16);  // word of step i0 - u
        } else {
            const uint32_t ra = bm_lane + ((uint32_t)(ii >> 5) << 8);
            if (u == 0 || u == 16) asm volatile("ds_read_b32 %0, %1" : "=v"(rd) : "v"(ra) : "memory");
            else asm volatile("ds_read_b32 %0, %1" : "=v"(rd) : "v"(ra));
        }
        const int slot = 30 - u;
        const uint32_t rv = ring[slot];
        ring[slot] = rv - ring[(slot + 28) % 31];
        const uint32_t j = sol_mod(I24, rv >> 1, mt[u], ii + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rd), "+v"(prev));
        if (POS) {
            if constexpr (u > 0) nw |= __builtin_amdgcn_ubfe(prev, pl.idx, 1) << (u - 1);
            prev = mskor_rtn(pos_addr(pl.base, j), pl.bit, rd & pl.bit);
        } else {
            if constexpr (u > 0) nw |= __builtin_amdgcn_ubfe(prev, ppos, 1) << (u - 1);
            const uint32_t bsp = (uint32_t)__builtin_amdgcn_sbfe((int)rd, ii & 31, 1);
            const uint32_t bit = 1u << (j & 31);
            uint32_t a;
            asm("v_lshl_add_u32 %0, %1, 8, %2" : "=v"(a) : "v"(j >> 5), "v"(bm_lane));
            prev = mskor_rtn(a, bit, bsp & bit);
            ppos = j;
        }
    });
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(prev) : : "memory");
    return nw | (__builtin_amdgcn_ubfe(prev, POS ? pl.idx : ppos, 1) << 30);
}

// the block straddling s and the one running below step 1, step by step (compiler-tracked)
template <bool POS>
__device__ __forceinline__ uint32_t sol_mixed(uint32_t (&ring)[31], uint32_t* bm, int lane,
                                              int half_words, int i0, int s,
                                              const uint64_t* __restrict__ mtab) {
    uint32_t word = 0;
    const uint32_t lbit = 1u << (lane & 31);
    uint32_t* bmh = bm + (lane >> 5) * half_words;
#pragma unroll
    for (int u = 0; u < 31; u++) {
        const int ii = i0 - u;
        const int slot = 30 - u;
        const uint32_t rv = ring[slot];
        ring[slot] = rv - ring[(slot + 28) % 31];
        if (ii < 1) continue;
        const uint32_t j = min(sol_mod(false, rv >> 1, mtab[ii + 1], ii + 1), (uint32_t)s);
        if (POS) {
            const uint32_t bi = ii < s ? bmh[ii] & lbit : 0u;
            const uint32_t old = atomicAnd(&bmh[j], ~lbit);
            if (ii < s) atomicOr(&bmh[j], bi);
            word |= __builtin_amdgcn_ubfe(old, lane & 31, 1) << u;
        } else {
            const uint32_t bi = ii < s ? (bm[(ii >> 5) * 64 + lane] >> (ii & 31)) & 1u : 0u;
            uint32_t* wp = &bm[(int)(j >> 5) * 64 + lane];
            const uint32_t old = atomicAnd(wp, ~(1u << (j & 31)));
            if (ii < s) atomicOr(wp, bi << (j & 31));
            word |= __builtin_amdgcn_ubfe(old, j, 1) << u;
        }
    }
    return word;
}

// V5 (POS, !FULL), V6 (POS, FULL), V7 (!POS, FULL), V8 / V9 (V5 / V6 + SPREAD).  nalloc: POS: position words per half (the
// allocation is 2 * nalloc words); else lane-major words per lane.  TAG only names the
// instantiation (V10 = V9 under its own kernel name, so that counters tell the two apart)
template <bool POS, bool FULL, bool SPREAD, int TAG = 0>
__global__ __launch_bounds__(64) void sol_pm_kernel(const int32_t* __restrict__ counts, int nwaves,
                                                    double frac, const uint64_t* __restrict__ mtab,
                                                    uint32_t* __restrict__ out, int nbw, int nalloc) {
    extern __shared__ uint32_t bm[];
    const int p = blockIdx.y, w = blockIdx.x, lane = threadIdx.x;
    const int M = counts[p];
    const int s = (int)(M * frac);
    if (POS) {
        for (int k = lane; k < nalloc; k += 64) bm[k] = bm[nalloc + k] = k < s ? ~0u : 0u;
        __syncthreads();
    } else {
        for (int k = 0; k < nalloc; k++)
            bm[k * 64 + lane] = k < (s >> 5) ? ~0u : k == (s >> 5) ? (1u << (s & 31)) - 1u : 0u;
    }
    uint32_t ring[31];
    uint32_t h = (uint32_t)(p * 7919 + w * 104729 + lane * 31337) | 1u;
#pragma unroll
    for (int t = 0; t < 31; t++) {
        h ^= h << 13; h ^= h >> 17; h ^= h << 5;
        ring[t] = h;
    }
    const uint32_t lds0 = (uint32_t)(size_t)(lds_u32*)bm;
    const uint32_t bm_lane = lds0 + 4u * (uint32_t)lane;
    PmLane pl;
    pl.base = lds0 + 4u * (uint32_t)((lane >> 5) * nalloc);
    pl.bit = 1u << (lane & 31);
    pl.nbit = ~pl.bit;
    pl.idx = (uint32_t)(lane & 31);
    pl.cap = (uint32_t)s + (SPREAD ? pl.idx : 0u);
    uint32_t* o = out + ((size_t)p * nwaves + w) * (size_t)nbw * 64 + lane;
    uint32_t acc = 0;
    int i = M - 1, b = 0;
    while (FULL ? i >= 1 : i - 30 >= 1) {
        uint32_t word;
        const bool i24 = i - 30 >= 255;
        if (!FULL || i - 30 >= s) {
            if (POS) word = i24 ? pm_draws<true>(ring, pl, i, s, mtab) : pm_draws<false>(ring, pl, i, s, mtab);
            else word = i24 ? sol_block<2, -1, true>(ring, bm_lane, i, s, mtab, acc)
                            : sol_block<2, -1, false>(ring, bm_lane, i, s, mtab, acc);
        } else if (i < s && i - 30 >= 1) {
            word = i24 ? sol_prefix<POS, true>(ring, pl, bm_lane, i, mtab)
                       : sol_prefix<POS, false>(ring, pl, bm_lane, i, mtab);
        } else {
            word = sol_mixed<POS>(ring, bm, lane, POS ? nalloc : 0, i, s, mtab);
        }
        o[(size_t)b * 64] = word;
        i -= 31;
        b++;
    }
    o[(size_t)b * 64] = acc ^ (uint32_t)i;
}

}  // namespace

extern "C" {
// n_pairs pairs with counts[p] matches (device), iterations -> grid; mtab = the magic table
// (device, d = 0 .. 65538: m_d | (l_d - 1) << 32); out = nbw words per lane (device).
// lds_bytes > 0: the dynamic LDS of the launch (>= what nalloc needs; V10), else derived from
// nalloc.  Returns the kernel time in ms (hipEvent), or -1 on an error.
float sol_run(int variant, const int32_t* counts, int n_pairs, int iters, double frac,
              const uint64_t* mtab, uint32_t* out, int nbw, int nalloc, int reps, int lds_bytes) {
    const int nwaves = (iters + 63) / 64;
    // V5 / V6 / V8 / V9: nalloc position words per half-wave; else nalloc words per lane
    const bool pm = variant == 5 || variant == 6 || variant == 8 || variant == 9 || variant == 10;
    const size_t need = pm ? (size_t)nalloc * 2 * 4 : (size_t)nalloc * 64 * 4;
    if (lds_bytes > 64 * 1024 || (lds_bytes > 0 && (size_t)lds_bytes < need)) return -1.f;
    const size_t shmem = lds_bytes > 0 ? (size_t)lds_bytes : need;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, 0);
    for (int r = 0; r < reps; r++) {
        switch (variant) {
#define SOL_L(V) case V: hipLaunchKernelGGL(sol_kernel<V>, dim3(nwaves, n_pairs), dim3(64), shmem, 0, \
                                             counts, nwaves, frac, mtab, out, nbw, nalloc); break;
            SOL_L(0) SOL_L(1) SOL_L(2) SOL_L(3) SOL_L(4)
#undef SOL_L
#define SOL_P(V, POS, FULL, SPREAD, ...) case V: hipLaunchKernelGGL((sol_pm_kernel<POS, FULL, SPREAD, ##__VA_ARGS__>),  \
                                                               dim3(nwaves, n_pairs), dim3(64), shmem, 0,  \
                                                               counts, nwaves, frac, mtab, out, nbw,       \
                                                               nalloc); break;
            SOL_P(5, true, false, false) SOL_P(6, true, true, false) SOL_P(7, false, true, false)
            SOL_P(8, true, false, true) SOL_P(9, true, true, true) SOL_P(10, true, true, true, 1)
#undef SOL_P
            default: return -1.f;
        }
    }
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return hipGetLastError() == hipSuccess ? ms / reps : -1.f;
}
}

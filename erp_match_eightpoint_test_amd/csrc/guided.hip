// guided.hip -- guided matching (include/erp_match.h "guided matching"; no reference
// counterpart): the descriptors of a packed batch rematched with each query's candidates
// restricted to the epipolar band |l^T E' r| < thr of a solved E.  It reads the batch, the result
// records and a solved 9-vector per pair and changes none of them; it draws no rand().
//
// Three launches:
//   guided_prep     one lane per train row: its bearing (fp64, and narrowed to fp32) into scratch
//                   and its claim word to all ones; the pair's first lane also E' = rank2_correct(e) and gated = 0.
//   guided_gate     the hot one.  256 threads, one lane per query, the pair's train rows through
//                   LDS in tiles of 64 (bearings fp64, descriptor rows fp32 at a 68-float stride).
//                   Per tile every lane builds its 64-bit pass mask -- an fp32 pre-test
//                   a32 . r32 with the margin of DESIGN.md 3.18 in a uniform loop whose train
//                   bearings come through scalar loads (wave-uniform addresses: SGPRs), then
//                   the defined fp64 residual for the survivors: the fp64 residual alone decides
//                   -- and the exact distances of the passed rows go through top2_consider in
//                   ascending j.  Two forms of the distance step (ERP_GUIDED_COMPACT):
//                     1  (shipped) a wave scan turns the masks into a per-wave item list in LDS,
//                        one lane per item computes exact_l2 (train row from LDS, the owner's
//                        query row from global memory: staging the query rows in LDS costs the
//                        occupancy), each owner folds its own items; a tile with
//                        more items than the list takes the per-lane loop;
//                     0  the per-lane loop only: each lane walks its own mask bits.
//                   Epilogue: the query's (j0, e0, e1, |G_i|) record, the integer add into gated
//                   and, for unique, the 64-bit atomicMin claim (bits(d0) << 32 | i) on row j0.
//   guided_compact  one workgroup per pair: ordered compaction of the accepted queries (that hold
//                   their claim) with the block scan of the matcher's merge -> matches, gathered
//                   keys, zeros up to max_nq, count, results_out, winners_out.
// The only atomics are the integer min and add above, whose results do not depend on the order:
// a pair's outputs are bit-identical from run to run and whatever else is in the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <type_traits>

#include "../../include/erp_match.h"
#include "erp_block.hpp"
#include "erp_ctx.hpp"
#include "erp_device.hpp"
#include "erp_l2.hpp"
#include "erp_launch.hpp"
#include "erp_stage.hpp"

// development variants (the _build.build(defines=...) route; DESIGN.md 3.18 has both timings)
#ifndef ERP_GUIDED_COMPACT
#define ERP_GUIDED_COMPACT 1
#endif
#ifndef ERP_GUIDED_PRETEST
#define ERP_GUIDED_PRETEST 1
#endif

using erp::CtxCall;

namespace {

using namespace erp;

constexpr float kInf = __builtin_huge_valf();
constexpr int kDim = 64;
constexpr int kGateThreads = 256;
constexpr int kGateWaves = kGateThreads / 64;
constexpr int kTile = 64;          // train rows per LDS tile: one bit of the pass mask each
constexpr int kRowStride = 68;     // floats per staged row: 16-lane b128 groups on distinct banks
constexpr int kItemList = 256;     // gated (query, row) items per wave and tile (more: per-lane loop)
constexpr int kCompactThreads = 1024;
constexpr int kXcds = 8;

// one query's outcome of the gate kernel
struct GuidedQuery {
    int32_t j0;      // -1: nothing gated (or no finite distance)
    float e0, e1;    // squared distances; +inf where there is none
    int32_t gated;   // |G_i|
};
static_assert(sizeof(GuidedQuery) == 16, "one 16-byte store per query");

struct GuidedArgs {
    erp_guided_inputs in;
    erp_guided_outputs out;
    double thr;
    float ratio, max_dist;
    int32_t unique;
    int32_t gate_blocks;           // gate workgroups per pair
    double* Ec;                    // [n_pairs][9]
    double* rb;                    // [n_pairs][max_nt][3]
    float4* rb32;                  // [n_pairs][max_nt] (+ one tile of slack): rb narrowed
    GuidedQuery* q;                // [n_pairs][max_nq]
    unsigned long long* claim;     // [n_pairs][max_nt]
};

// rule 7: the result's status first, then the source's (no match count: the batch bounds the rows)
__device__ __forceinline__ int32_t pair_status(const GuidedArgs& a, int p) {
    return stage_gate(a.in.results ? a.in.results[p].status : (int32_t)ERP_OK, 0,
                      source_of(a.in).status_of(p));
}

// the pair's row counts, never above the bounds the scratch was sized for
__device__ __forceinline__ void pair_rows(const GuidedArgs& a, int p, int* nq, int* nt) {
    const int64_t q = a.in.batch.off_l[p + 1] - a.in.batch.off_l[p];
    const int64_t t = a.in.batch.off_r[p + 1] - a.in.batch.off_r[p];
    *nq = (int)(q < 0 ? 0 : (q > a.in.batch.max_nq ? a.in.batch.max_nq : q));
    *nt = (int)(t < 0 ? 0 : (t > a.in.batch.max_nt ? a.in.batch.max_nt : t));
}

// rules 3 and 4 from a query's record: accepted or not, d0 out
__device__ __forceinline__ bool guided_accept(const GuidedArgs& a, const GuidedQuery& r, float* d0) {
    *d0 = __builtin_sqrtf(r.e0);
    const float d1 = __builtin_sqrtf(r.e1);
    return r.gated >= 1 && r.j0 >= 0 && *d0 < a.ratio * d1 && (!(a.max_dist > 0) || *d0 < a.max_dist);
}

__global__ __launch_bounds__(256) void guided_prep_kernel(GuidedArgs a) {
    const int blocks = (int)(gridDim.x / (unsigned)a.in.batch.n_pairs);
    const int p = blockIdx.x / blocks, j = (blockIdx.x % blocks) * 256 + threadIdx.x;
    int nq, nt;
    pair_rows(a, p, &nq, &nt);
    if (j == 0) {
        if (a.out.gated) a.out.gated[p] = 0;
        if (pair_status(a, p) == ERP_OK) {
            const double* e = source_of(a.in).e_of(p);
            double e9[9], Ec[9];
#pragma unroll
            for (int k = 0; k < 9; k++) e9[k] = e[k];
            rank2_correct(e9, Ec);
#pragma unroll
            for (int k = 0; k < 9; k++) a.Ec[(size_t)p * 9 + k] = Ec[k];
        }
    }
    if (j >= nt) return;
    const size_t row = (size_t)p * a.in.batch.max_nt + j;
    const erp_point2f k = a.in.batch.kp_r[a.in.batch.off_r[p] + j];
    double b[3];
    pixel_to_bearing(a.in.batch.width[p], a.in.batch.height[p], k.x, k.y, b);
    a.rb[row * 3] = b[0];
    a.rb[row * 3 + 1] = b[1];
    a.rb[row * 3 + 2] = b[2];
    a.rb32[row] = make_float4((float)b[0], (float)b[1], (float)b[2], 0.f);
    a.claim[row] = ~0ull;
}

// orders a wave's own LDS stores before its later LDS loads from other lanes' addresses (the
// item list is per wave: no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the gate kernel's LDS; the item list only in the compacted form
struct GateTile {
    double r64[kTile * 3];
    float row[kTile * kRowStride];
};
struct GateItems {
    float e[kGateWaves][kItemList];
    uint16_t item[kGateWaves][kItemList];
};
struct GateNoItems {};

// (held to 128 VGPRs: 4 waves per SIMD)
#define ERP_GUIDED_GATE_WAVES __attribute__((amdgpu_waves_per_eu(4)))
template <bool kCompact, bool kPretest>
__global__ __launch_bounds__(kGateThreads) ERP_GUIDED_GATE_WAVES void guided_gate_kernel(GuidedArgs a) {
    __shared__ __attribute__((aligned(16))) GateTile ts;
    __shared__ __attribute__((aligned(16))) std::conditional_t<kCompact, GateItems, GateNoItems> is;

    // a pair's workgroups on one XCD (workgroup ids go round the 8 XCDs): its train rows then
    // come through one L2 instead of eight
    const int per_xcd = (int)(gridDim.x / kXcds);
    const int64_t lin = (int64_t)(blockIdx.x % kXcds) * per_xcd + blockIdx.x / kXcds;
    if (lin >= (int64_t)a.in.batch.n_pairs * a.gate_blocks) return;
    const int p = (int)(lin / a.gate_blocks), q0 = (int)(lin % a.gate_blocks) * kGateThreads;
    int nq, nt;
    pair_rows(a, p, &nq, &nt);
    if (q0 >= nq || nt == 0 || pair_status(a, p) != ERP_OK) return;  // (block-uniform)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = q0 + tid;
    const bool valid = i < nq;
    const int W = a.in.batch.width[p], H = a.in.batch.height[p];
    const float* dt = a.in.batch.desc_r + (size_t)a.in.batch.off_r[p] * kDim;
    const double* rb = a.rb + (size_t)p * a.in.batch.max_nt * 3;
    // (read with wave-uniform indices only: scalar loads, the rows of a tile arrive in SGPRs)
    const float4* __restrict__ rb32 = a.rb32 + (size_t)p * a.in.batch.max_nt;

    double Ec[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Ec[k] = a.Ec[(size_t)p * 9 + k];

    // the query: its descriptor row (in registers; the compacted form reads query rows from
    // global memory, whichever lane computes the item) and its bearing
    const float4* qrows = reinterpret_cast<const float4*>(
        a.in.batch.desc_l + (size_t)(a.in.batch.off_l[p] + q0) * kDim);  // this workgroup's rows
    float4 qreg[kCompact ? 1 : 16];
    const float4* qr = qrows + (size_t)(valid ? tid : 0) * 16;
    if constexpr (!kCompact) {
#pragma unroll
        for (int c = 0; c < 16; c++) qreg[c] = qr[c];
        qr = qreg;
    }
    double l[3];
    {
        const erp_point2f k = a.in.batch.kp_l[a.in.batch.off_l[p] + (valid ? i : q0)];
        pixel_to_bearing(W, H, k.x, k.y, l);
    }
    // the fp32 pre-test: res = a . r with a = E'^T l; |fp32(a32 . r32) - a . r| <= 5.01 u S with
    // u = 2^-24, S = sum |a_k| (|r_k| <= 1), and the fp64 roundings of a and of the defined
    // residual stay under 2^-46 N, N = sum |E'_k| -- DESIGN.md 3.18 -- so a row with |res| < thr
    // has |pre| < thr + 8 u S + 2^-46 N.  `always`: a lane whose a is too large for the bound
    // (or not finite) sends every row to the fp64 residual.
    float a32[3] = {0.f, 0.f, 0.f}, t32 = 0.f;
    bool always = true;
    if constexpr (kPretest) {
        double ad[3];
#pragma unroll
        for (int c = 0; c < 3; c++) ad[c] = (Ec[c] * l[0] + Ec[3 + c] * l[1]) + Ec[6 + c] * l[2];
        const double S = (fabs(ad[0]) + fabs(ad[1])) + fabs(ad[2]);
        double N = 0.0;
#pragma unroll
        for (int k = 0; k < 9; k++) N += fabs(Ec[k]);
        always = !(S < 1e30);
        const double lim = ((a.thr + S * (8.0 / 16777216.0)) + N * 0x1p-46) + 1e-30;
        t32 = (float)lim * 1.000001f;  // (the narrowing rounds either way)
#pragma unroll
        for (int c = 0; c < 3; c++) a32[c] = (float)ad[c];
    }

    float b0 = kInf, b1 = kInf;
    int j0 = -1, gated = 0;

    for (int t0 = 0; t0 < nt; t0 += kTile) {
        const int rows = min(kTile, nt - t0);
        __syncthreads();  // the previous tile is folded
        if (tid < kTile) {
            double r[3] = {0.0, 0.0, 0.0};
            if (tid < rows) {
#pragma unroll
                for (int k = 0; k < 3; k++) r[k] = rb[(size_t)(t0 + tid) * 3 + k];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) ts.r64[tid * 3 + k] = r[k];
        }
#pragma unroll
        for (int m = 0; m < kTile * 16 / kGateThreads; m++) {
            const int k = tid + m * kGateThreads, row = k >> 4, c = k & 15;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < rows) v = reinterpret_cast<const float4*>(dt + (size_t)(t0 + row) * kDim)[c];
            *reinterpret_cast<float4*>(&ts.row[row * kRowStride + c * 4]) = v;
        }
        __syncthreads();

        // ---- the pass mask of this lane over the tile's rows ----
        uint64_t mask = 0;
        if constexpr (kPretest) {
#pragma unroll 1
            for (int g = 0; g < kTile / 16; g++) {  // 16 rows per step keeps the loads in few VGPRs
                uint32_t m16 = 0u;
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const float4 rv = rb32[t0 + g * 16 + b];  // (past nt: masked below)
                    const float pre = __builtin_fmaf(
                        a32[2], rv.z, __builtin_fmaf(a32[1], rv.y, a32[0] * rv.x));
                    m16 |= (!(fabsf(pre) >= t32) ? 1u : 0u) << b;
                }
                mask |= (uint64_t)m16 << (g * 16);
            }
            if (always) mask = ~0ull;
            if (rows < kTile) mask &= (1ull << rows) - 1;
            if (!valid) mask = 0;
            uint64_t todo = mask;
            while (todo) {  // the survivors: the defined residual decides
                const int jj = __builtin_ctzll(todo);
                todo &= todo - 1;
                if (!(fabs(inlier_residual(Ec, l, &ts.r64[jj * 3])) < a.thr)) mask &= ~(1ull << jj);
            }
        } else {
            for (int jj = 0; jj < rows; jj++)
                if (fabs(inlier_residual(Ec, l, &ts.r64[jj * 3])) < a.thr) mask |= 1ull << jj;
            if (!valid) mask = 0;
        }
        const int mine = __popcll(mask);
        gated += mine;

        // ---- the exact distances of the passed rows, folded in ascending j ----
        bool listed = false;
        int first = 0, total = 0;
        if constexpr (kCompact) {
            const int x = wave_inclusive_scan(mine, lane);
            total = __shfl(x, 63, 64);
            first = x - mine;
            listed = total <= kItemList;  // (wave-uniform)
            if (listed) {
                uint64_t todo = mask;
                for (int k = first; todo; k++) {
                    is.item[wave][k] = (uint16_t)((lane << 6) | __builtin_ctzll(todo));
                    todo &= todo - 1;
                }
            }
            wave_lds_sync();  // the wave's items are listed
            if (listed) {
                for (int k = lane; k < total; k += 64) {
                    const int it = is.item[wave][k];
                    is.e[wave][k] = exact_l2(
                        qrows + (size_t)(wave * 64 + (it >> 6)) * 16,
                        reinterpret_cast<const float4*>(&ts.row[(it & 63) * kRowStride]));
                }
            }
        }
        if (!listed) {
            uint64_t todo = mask;
            while (todo) {
                const int jj = __builtin_ctzll(todo);
                todo &= todo - 1;
                top2_consider(exact_l2(qr, reinterpret_cast<const float4*>(&ts.row[jj * kRowStride])),
                              t0 + jj, b0, j0, b1);
            }
        }
        if constexpr (kCompact) {
            wave_lds_sync();  // the items' distances are there
            if (listed) {  // each owner folds its own items in ascending j
                uint64_t todo = mask;
                for (int k = first; todo; k++) {
                    top2_consider(is.e[wave][k], t0 + __builtin_ctzll(todo), b0, j0, b1);
                    todo &= todo - 1;
                }
            }
        }
    }

    // ---- epilogue: the record, gated, the claim ----
    unsigned long long gsum = (unsigned long long)gated;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o, 64);
    if (lane == 0 && a.out.gated && gsum)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.out.gated + p), gsum);
    if (!valid) return;
    const GuidedQuery rec{j0, b0, b1, gated};
    a.q[(size_t)p * a.in.batch.max_nq + i] = rec;
    float d0;
    if (a.unique && guided_accept(a, rec, &d0))
        atomicMin(a.claim + (size_t)p * a.in.batch.max_nt + j0,
                  ((unsigned long long)__float_as_uint(d0) << 32) | (unsigned)i);
}

static_assert(sizeof(erp_winner) == 88, "guided_compact_kernel writes 11 words");

__global__ __launch_bounds__(kCompactThreads) void guided_compact_kernel(GuidedArgs a) {
    __shared__ int ws[kCompactThreads / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int max_nq = a.in.batch.max_nq;
    const int32_t status = pair_status(a, p);
    int nq, nt;
    pair_rows(a, p, &nq, &nt);
    if (status != ERP_OK || nt == 0) nq = 0;  // (the gate kernel wrote no records then)

    erp_dmatch* mo = a.out.matches ? a.out.matches + (size_t)p * max_nq : nullptr;
    erp_point2f* klo = a.out.key_left ? a.out.key_left + (size_t)p * max_nq : nullptr;
    erp_point2f* kro = a.out.key_right ? a.out.key_right + (size_t)p * max_nq : nullptr;
    const GuidedQuery* qrec = a.q + (size_t)p * max_nq;
    const unsigned long long* claim = a.claim + (size_t)p * a.in.batch.max_nt;
    const int64_t ol = a.in.batch.off_l[p], orr = a.in.batch.off_r[p];

    int base = 0;
    for (int c0 = 0; c0 < nq; c0 += kCompactThreads) {  // (block-uniform bounds)
        const int i = c0 + tid;
        bool keep = false;
        float d0 = 0.f;
        int j0 = 0;
        if (i < nq) {
            const GuidedQuery r = qrec[i];
            j0 = r.j0;
            keep = guided_accept(a, r, &d0);
            if (keep && a.unique) keep = (uint32_t)claim[j0] == (uint32_t)i;
        }
        int total;
        const int m = base + block_exclusive_scan<kCompactThreads>(keep ? 1 : 0, ws, &total);
        if (keep) {
            if (mo) mo[m] = erp_dmatch{i, j0, 0, d0};
            if (klo) klo[m] = a.in.batch.kp_l[ol + i];
            if (kro) kro[m] = a.in.batch.kp_r[orr + j0];
        }
        base += total;
    }
    for (int m = base + tid; m < max_nq; m += kCompactThreads) {
        if (mo) mo[m] = erp_dmatch{0, 0, 0, 0.f};
        if (klo) klo[m] = erp_point2f{0.f, 0.f};
        if (kro) kro[m] = erp_point2f{0.f, 0.f};
    }
    __syncthreads();  // every read of the result record is done (results_out may be the input)
    if (tid != 0) return;
    a.out.count[p] = base;
    if (a.out.results_out)  // M replaced
        copy_result(a.out.results_out + p, a.in.results + p, [=](uint64_t* w) {
            w[3] = (w[3] & 0xffffffffull) | ((uint64_t)(uint32_t)base << 32);
        });
    if (a.out.winners_out) {
        erp_winner o = stage_record<erp_winner>(status);
        if (status == ERP_OK) {
            o.iter = -1;
            const double* e = source_of(a.in).e_of(p);
#pragma unroll
            for (int k = 0; k < 9; k++) o.E[k] = e[k];
        }
        a.out.winners_out[p] = o;
    }
}

}  // namespace

extern "C" {

erp_status erp_match_guided_dev(erp_ctx* ctx, const erp_guided_inputs* in,
                                const erp_guided_cfg* cfg, const erp_guided_outputs* out,
                                void* stream) {
    if (!ctx || !in || !cfg || !out || !out->count || in->batch.n_pairs < 0) return ERP_INVALID_ARG;
    const erp_pair_batch& b = in->batch;
    if (!(cfg->thr > 0) || !(cfg->ratio > 0) || std::isnan(cfg->max_dist) || b.dim != kDim ||
        b.max_nq < 0 || b.max_nt < 0 || b.max_nq > kStageMaxM)
        return ERP_INVALID_ARG;
    if (b.n_pairs == 0) return ERP_OK;
    if (!b.desc_l || !b.desc_r || !b.kp_l || !b.kp_r || !b.off_l || !b.off_r || !b.width ||
        !b.height || !source_ok(source_of(*in)) || (!in->results && out->results_out))
        return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    const size_t P = (size_t)b.n_pairs;
    GuidedArgs a{};
    a.in = *in;
    a.out = *out;
    a.thr = (double)cfg->thr;
    a.ratio = cfg->ratio;
    a.max_dist = cfg->max_dist;
    a.unique = cfg->unique;
    a.gate_blocks = (b.max_nq + kGateThreads - 1) / kGateThreads;
    a.q = ctx_scratch<GuidedQuery>(ctx, kSlotGuidedQuery, P * b.max_nq * sizeof(GuidedQuery));
    a.claim = ctx_scratch<unsigned long long>(ctx, kSlotGuidedClaim, P * b.max_nt * 8);
    // the narrowed bearings first (16-byte aligned), with one tile of slack: the pre-test reads
    // whole tiles
    const size_t n32 = P * b.max_nt + kTile;
    a.rb32 = ctx_scratch<float4>(ctx, kSlotGuidedBearings,
                                 n32 * 16 + P * ((size_t)b.max_nt * 3 + 9) * 8);
    if (!a.q || !a.claim || !a.rb32) return ERP_OUT_OF_MEMORY;
    a.Ec = (double*)(a.rb32 + n32);
    a.rb = a.Ec + P * 9;
    const unsigned prep_blocks = (unsigned)std::max(1, (b.max_nt + 255) / 256);
    ERP_LAUNCH_S(guided_prep_kernel, dim3((unsigned)P * prep_blocks), dim3(256), 0, st, a);
    if (a.gate_blocks > 0 && b.max_nt > 0) {
        const size_t per_xcd = (P * a.gate_blocks + kXcds - 1) / kXcds;
        ERP_LAUNCH_S((guided_gate_kernel<ERP_GUIDED_COMPACT != 0, ERP_GUIDED_PRETEST != 0>),
                     dim3((unsigned)(per_xcd * kXcds)), dim3(kGateThreads), 0, st, a);
    }
    ERP_LAUNCH_S(guided_compact_kernel, dim3((unsigned)P), dim3(kCompactThreads), 0, st, a);
    return hipGetLastError() == hipSuccess ? ERP_OK : ERP_HIP_ERROR;
}

erp_status erp_match_guided(erp_ctx* ctx, const float* h_desc1, int32_t n1, const float* h_desc2,
                            int32_t n2, const erp_point2f* h_kp1, const erp_point2f* h_kp2,
                            int32_t W, int32_t H, const double E[9], const erp_guided_cfg* cfg,
                            erp_dmatch* h_out, int32_t* h_count) {
    if (!ctx || !cfg || !E || !h_count || n1 < 0 || n2 < 0 || n1 > kStageMaxM || W <= 0 || H <= 0 ||
        (n1 > 0 && (!h_desc1 || !h_kp1 || !h_out)) || (n2 > 0 && (!h_desc2 || !h_kp2)))
        return ERP_INVALID_ARG;
    *h_count = 0;
    // one lock across upload, match and download: the staging buffer is the context's
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    const GuidedStage L(n1, n2);
    char* base = ctx_scratch<char>(ctx, kSlotHostStage, L.bytes);
    if (!base) return ERP_OUT_OF_MEMORY;
    const int64_t off[4] = {0, n1, 0, n2};
    const int32_t wh[2] = {W, H};
    ERP_CK(hipMemcpy(base + L.e, E, 72, hipMemcpyHostToDevice));
    ERP_CK(hipMemcpy(base + L.off, off, sizeof(off), hipMemcpyHostToDevice));
    ERP_CK(hipMemcpy(base + L.wh, wh, sizeof(wh), hipMemcpyHostToDevice));
    if (n1 > 0) {
        ERP_CK(hipMemcpy(base + L.desc1, h_desc1, (size_t)n1 * kDim * 4, hipMemcpyHostToDevice));
        ERP_CK(hipMemcpy(base + L.kp1, h_kp1, (size_t)n1 * 8, hipMemcpyHostToDevice));
    }
    if (n2 > 0) {
        ERP_CK(hipMemcpy(base + L.desc2, h_desc2, (size_t)n2 * kDim * 4, hipMemcpyHostToDevice));
        ERP_CK(hipMemcpy(base + L.kp2, h_kp2, (size_t)n2 * 8, hipMemcpyHostToDevice));
    }
    erp_guided_inputs in{};
    in.batch.n_pairs = 1;
    in.batch.dim = kDim;
    in.batch.max_nq = n1;
    in.batch.max_nt = n2;
    in.batch.desc_l = (const float*)(base + L.desc1);
    in.batch.desc_r = (const float*)(base + L.desc2);
    in.batch.kp_l = (const erp_point2f*)(base + L.kp1);
    in.batch.kp_r = (const erp_point2f*)(base + L.kp2);
    in.batch.off_l = (const int64_t*)(base + L.off);
    in.batch.off_r = in.batch.off_l + 2;
    in.batch.width = (const int32_t*)(base + L.wh);
    in.batch.height = in.batch.width + 1;
    in.e = base + L.e;
    in.e_stride = 72;
    erp_guided_outputs out{};
    out.count = (int32_t*)(base + L.count);
    out.matches = (erp_dmatch*)(base + L.matches);
    const erp_status s = erp_match_guided_dev(ctx, &in, cfg, &out, nullptr);
    if (s != ERP_OK) return s;
    ERP_CK(hipDeviceSynchronize());
    int32_t m = 0;
    ERP_CK(hipMemcpy(&m, out.count, 4, hipMemcpyDeviceToHost));
    if (m > 0) ERP_CK(hipMemcpy(h_out, out.matches, (size_t)m * sizeof(erp_dmatch), hipMemcpyDeviceToHost));
    *h_count = m;
    return ERP_OK;
}

}  // extern "C"

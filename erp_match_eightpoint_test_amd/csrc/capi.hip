// capi.hip -- the C ABI declared in include/erp_match.h: context, device scratch and the
// orchestration of the hot-path kernels on one HIP stream.  No host round trip inside a
// pipeline run (match counts, sample sizes and hypothesis counts stay on the device).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/erp_match.h"
#include "erp_ctx.hpp"
#include "erp_kernels.hpp"

// eigen stage fused into the Gram kernel (kernels.hip gram_mfma_kernel: no Gram round trip
// through HBM for the common s >= 9 pairs): 1 = the inverse iteration, 2 = and the estimate;
// 0 = the separate eigen_kernel / estimate_kernel, for A/B
#ifndef ERP_FUSE_EIGEN
#define ERP_FUSE_EIGEN 1
#endif
// hypothesis records' E written only when the caller asked for the records (out->hyps)
#ifndef ERP_SKIP_E
#define ERP_SKIP_E 1
#endif

namespace {

// Debug: erp_debug_set_alloc_pad(N) gives every buffer allocated afterwards N canary bytes
// (0xA5) past its end; erp_debug_check_pads() reports buffers whose canary a kernel overwrote.
std::atomic<size_t> g_alloc_pad{0};
size_t alloc_pad() { return g_alloc_pad.load(std::memory_order_relaxed); }
std::mutex g_pad_mu;
std::vector<std::pair<void*, size_t>> g_padded;

}  // namespace

namespace erp {

void free_buf(DevBuf& b) {
    if (!b.p) return;
    if (alloc_pad()) {
        std::lock_guard<std::mutex> g(g_pad_mu);
        const auto it = std::find_if(g_padded.begin(), g_padded.end(),
                                     [&](const std::pair<void*, size_t>& e) { return e.first == b.p; });
        if (it != g_padded.end()) g_padded.erase(it);
    }
    (void)hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
}

bool ensure(DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.n >= bytes) return true;
    const size_t pad = alloc_pad();
    if (b.p) free_buf(b);
    b.p = nullptr;
    b.n = 0;
    if (hipMalloc(&b.p, bytes + pad) != hipSuccess) return false;
    if (pad) {
        if (hipMemset((char*)b.p + bytes, 0xA5, pad) != hipSuccess) return false;
        std::lock_guard<std::mutex> g(g_pad_mu);
        g_padded.emplace_back(b.p, bytes);
    }
    b.n = bytes;
    return true;
}

}  // namespace erp

using erp::CtxCall;
using erp::DevBuf;
using erp::HostCtxCall;
using erp::RsTurn;
using erp::StageTimer;

// every named DevBuf of the context (extra[] and snap apart); graph = a captured
// erp_pair_batch_run bakes its address in (graph_key).  The host-pointer entry points' staging
// (off, wh, in_a..in_d) is not part of that call.
struct CtxBuf {
    DevBuf erp_ctx::*m;
    bool graph;
};
#define ERP_B(name, graph) {&erp_ctx::name, graph}
const CtxBuf kCtxBufs[] = {
    ERP_B(mblk, 1), ERP_B(zsel, 1), ERP_B(part, 1), ERP_B(part1, 1), ERP_B(pu, 1),
    ERP_B(ccount, 1), ERP_B(cand, 1), ERP_B(bsel, 1), ERP_B(edges, 1), ERP_B(gfin, 1),
    ERP_B(matches, 1), ERP_B(counts, 1), ERP_B(flags, 1), ERP_B(pts, 1), ERP_B(polyR, 1),
    ERP_B(polyQ, 1), ERP_B(idx, 1), ERP_B(gram, 1), ERP_B(hyps, 1), ERP_B(rv, 1), ERP_B(tv, 1),
    ERP_B(kcount, 1), ERP_B(tmean, 1), ERP_B(sortbuf, 1), ERP_B(w0, 1), ERP_B(off, 0),
    ERP_B(wh, 0), ERP_B(results, 1), ERP_B(in_a, 0), ERP_B(in_b, 0), ERP_B(in_c, 0),
    ERP_B(in_d, 0), ERP_B(dscale, 1), ERP_B(lb, 1), ERP_B(ub, 1), ERP_B(surv, 1),
    ERP_B(nsurv, 1), ERP_B(wins, 1), ERP_B(rtab, 1), ERP_B(limbs, 1), ERP_B(tsplit, 1),
    ERP_B(ovf, 1), ERP_B(vchunk, 1), ERP_B(lipref, 1), ERP_B(inl, 1), ERP_B(hlite, 1),
    ERP_B(w0s, 1), ERP_B(rep, 1)};
#undef ERP_B

extern "C" {

int32_t erp_abi_version(void) { return ERP_MATCH_ABI_VERSION; }

const char* erp_status_string(erp_status s) {
    switch (s) {
        case ERP_OK: return "ok";
        case ERP_INVALID_ARG: return "invalid argument";
        case ERP_TOO_FEW_POINTS: return "too few points";
        case ERP_NO_VALID_HYPOTHESIS: return "no valid rotation hypothesis";
        case ERP_HIP_ERROR: return "HIP error";
        case ERP_NO_DEVICE: return "no HIP device";
        case ERP_OUT_OF_MEMORY: return "out of device memory";
        case ERP_INTERNAL: return "internal consistency check failed";
    }
    return "unknown";
}

void erp_ransac_cfg_default(erp_ransac_cfg* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->iters = 80;
    cfg->sampler = ERP_SAMPLER_GLIBC;
    cfg->sample_frac = 0.25;
    cfg->trim_lo = 0.2;
    cfg->trim_hi = 0.8;
    cfg->valid_abs = 1.57;
    cfg->seed = 1;
    cfg->offset = 0;
}

erp_status erp_ctx_create(int32_t device, erp_ctx** out) {
    if (!out) return ERP_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ERP_NO_DEVICE;
    if (device < 0 || device >= n) return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(device));
    erp_ctx* c = new (std::nothrow) erp_ctx();
    if (!c) return ERP_OUT_OF_MEMORY;
    c->device = device;
    erp::init_constants();
    erp::init_stream_constants();
    *out = c;
    return ERP_OK;
}

erp_status erp_ctx_destroy(erp_ctx* ctx) {
    if (!ctx) return ERP_INVALID_ARG;
    (void)hipSetDevice(ctx->device);
    for (const CtxBuf& b : kCtxBufs) free_buf(ctx->*b.m);
    for (DevBuf& b : ctx->extra) free_buf(b);
    free_buf(ctx->snap);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->done) (void)hipEventDestroy(ctx->done);
    for (auto& g : ctx->graphs) (void)hipGraphExecDestroy(g.exec);
    delete ctx;
    return ERP_OK;
}

}  // extern "C"

namespace {

erp::BatchShape make_shape(int n_pairs, int max_nq, int max_nt, int iters, double frac) {
    erp::BatchShape sh{};
    sh.n_pairs = n_pairs;
    sh.max_nq = std::max(max_nq, 1);
    sh.max_nt = std::max(max_nt, 1);
    // matcher filter grid: 256 queries x one train chunk per block, >= ~1024 blocks, chunks of
    // >= 256 rows (the filter's first stage of every chunk runs twice, bounds then candidates)
    const int qblocks = (sh.max_nq + 255) / 256;
    const int tmax = std::max(1, (sh.max_nt + 255) / 256);
    int chunks = (1024 + qblocks * n_pairs - 1) / (qblocks * n_pairs);
    chunks = std::max(1, std::min(chunks, tmax));
    int chunk_len = (sh.max_nt + chunks - 1) / chunks;
    chunk_len = (chunk_len + 31) / 32 * 32;
    sh.fchunk_len = chunk_len;
    sh.fchunks = (sh.max_nt + chunk_len - 1) / chunk_len;
    // exact VALU sweep: 128 queries x one chunk (multiple of 128 train rows) per block
    const int xqblocks = (sh.max_nq + 127) / 128;
    int xch = (2048 + xqblocks * n_pairs - 1) / (xqblocks * n_pairs);
    xch = std::max(1, std::min(xch, (sh.max_nt + 127) / 128));
    sh.xchunk_len = ((sh.max_nt + xch - 1) / xch + 127) / 128 * 128;
    sh.xchunks = (sh.max_nt + sh.xchunk_len - 1) / sh.xchunk_len;
    sh.iters = std::max(iters, 1);
    sh.max_s = std::max((int)(sh.max_nq * frac), 1);
    sh.idx_stride = sh.max_s;
    sh.sel_words = (sh.max_nq + 30) / 31 + 1;
    return sh;
}

bool ensure_matcher(erp_ctx* c, const erp::BatchShape& sh) {
    const size_t PQ = (size_t)sh.n_pairs * sh.max_nq;
    const size_t fold = PQ * sizeof(erp::Top2);
    if (!ensure(c->mblk, erp::knn2_merge_scratch_bytes(sh))) return false;
    if (c->matcher == ERP_MATCHER_VALU_EXACT)
        return ensure(c->part, PQ * sh.xchunks * sizeof(erp::Top2)) && ensure(c->part1, fold);
    return ensure(c->part, PQ * sh.fchunks * sizeof(erp::Top2)) && ensure(c->part1, fold) &&
           ensure(c->pu, PQ * sh.fchunks * sizeof(float2) + PQ * sizeof(float)) &&  // + |q|^2
           ensure(c->ccount, PQ * sh.fchunks * 2 * 4) &&
           ensure(c->cand, erp::knn2_cand_bytes(sh)) &&
           ensure(c->tsplit, erp::knn2_split_bytes(sh)) &&
           ensure(c->ovf, 4 + 12 * PQ * sh.fchunks);
}

// per-chunk partials -> (fold when there are several chunks) -> ratio test + compaction
// bo != nullptr: the merge also gathers the matched keypoints and writes their bearings
// (bearings_from_matches_kernel's work, one launch fewer)
erp_status fold_and_merge(erp_ctx* ctx, const int64_t* oq, const int64_t* ot,
                          const erp::BatchShape& sh, int chunk_len, int chunks, float ratio,
                          erp_dmatch* matches, int32_t* counts, int32_t* flags, hipStream_t st,
                          const erp::BearingOut* bo = nullptr) {
    StageTimer _t(ctx, ERP_STAGE_KNN2_MERGE, st);
    const erp::Top2* part = (const erp::Top2*)ctx->part.p;
    if (chunks > 1) {
        ERP_CK(erp::launch_knn2_fold(part, oq, ot, sh, chunk_len, chunks, (erp::Top2*)ctx->part1.p,
                                     st));
        part = (const erp::Top2*)ctx->part1.p;
    }
    // a single chunk spanning the whole train set
    ERP_CK(erp::launch_knn2_merge(part, oq, ot, sh, sh.max_nt, 1, ratio, matches, counts, flags,
                                  (int32_t*)ctx->mblk.p, st, bo));
    return ERP_OK;
}

// exact k=2 + ratio test: MFMA filter (bounds + provisional candidates), exact rescoring, merge -- or
// the exact packed-FP32 sweep, merge
erp_status run_matcher(erp_ctx* ctx, const float* dq, const float* dt, const int64_t* oq,
                       const int64_t* ot, const erp::BatchShape& sh, float ratio,
                       erp_dmatch* matches, int32_t* counts, int32_t* flags, hipStream_t st,
                       const erp::BearingOut* bo = nullptr) {
    if (ctx->matcher == ERP_MATCHER_VALU_EXACT) {
        {
            StageTimer _t(ctx, ERP_STAGE_KNN2_EXACT, st);
            ERP_CK(erp::launch_knn2_exact(dq, dt, oq, ot, sh, (erp::Top2*)ctx->part.p, st));
        }
        return fold_and_merge(ctx, oq, ot, sh, sh.xchunk_len, sh.xchunks, ratio, matches, counts,
                              flags, st, bo);
    }
    auto* pu = (float2*)ctx->pu.p;
    auto* cc = (int32_t*)ctx->ccount.p;
    void* cand = ctx->cand.p;
    {
        StageTimer _t(ctx, ERP_STAGE_KNN2_FILTER, st);
        ERP_CK(erp::launch_knn2_filter(dq, dt, oq, ot, sh, ctx->tsplit.p, pu, cc, cand, st,
                                       (int32_t*)ctx->ovf.p, flags));
    }
    {
        StageTimer _t(ctx, ERP_STAGE_KNN2_RESCORE, st);
        ERP_CK(erp::launch_knn2_rescore(dq, dt, oq, ot, sh, ctx->tsplit.p, pu, cc, cand,
                                        (erp::Top2*)ctx->part.p, (int32_t*)ctx->ovf.p,
                                        ctx->opt[ERP_OPT_BOUND_RATIO] ? ratio : -1.f, st));
    }
    return fold_and_merge(ctx, oq, ot, sh, sh.fchunk_len, sh.fchunks, ratio, matches, counts,
                          flags, st, bo);
}

erp_status ensure_estimator(erp_ctx* c, const erp::BatchShape& sh, const erp_batch_outputs* out) {
    const size_t P = (size_t)sh.n_pairs;
    const size_t nwaves = (size_t)(sh.iters + 63) / 64;
    const erp::ConsensusLayout L = erp::consensus_layout(sh.n_pairs, sh.iters);
    bool ok = ensure(c->counts, P * 4) && ensure(c->flags, P * 4) && ensure(c->rep, P * 4) &&
              ensure(c->pts, P * (sh.max_nq + 1) * 48) &&
              ensure(c->wins, P * nwaves * 31 * 64 * 4) && ensure(c->polyR, P * 65 * 31 * 4) &&
              ensure(c->polyQ, P * erp::kMaxQ * 31 * 4) &&
              ensure(c->idx, P * nwaves * (size_t)sh.sel_words * 64 * 4) &&
              ensure(c->gram, P * sh.iters * 36 * 8) && ensure(c->limbs, erp::gram_limbs_bytes(sh)) &&
              ensure(c->gfin, P * sh.iters * 9 * 8) && ensure(c->rv, P * 6 * sh.iters * 4) &&
              ensure(c->kcount, P * 4) && ensure(c->sortbuf, L.sortbuf.bytes) &&
              ensure(c->w0, 31 * 4) && ensure(c->results, P * sizeof(erp_pair_result)) &&
              ensure(c->dscale, P * 4) && ensure(c->lb, L.lb_bytes) && ensure(c->ub, L.ub_bytes) &&
              ensure(c->surv, L.surv_bytes) && ensure(c->bsel, L.bsel_bytes) &&
              ensure(c->zsel, L.zsel_bytes) && ensure(c->lipref, L.lipref.bytes) &&
              ensure(c->edges, L.edges.bytes) && ensure(c->nsurv, L.counts.bytes) &&
              ensure(c->vchunk, erp::valid_chunk_bytes(sh));
    if (ok && !(out && out->hyps)) ok = ensure(c->hyps, P * sh.iters * sizeof(erp_hypothesis));
    if (ok) ok = ensure(c->hlite, L.hlite.bytes);
    if (ok && !(out && out->tvec)) ok = ensure(c->tv, P * 6 * sh.iters * 4);
    if (ok && !(out && out->dist)) ok = ensure(c->tmean, P * 2 * sh.iters * 8);
    if (!ok) return ERP_OUT_OF_MEMORY;
    if (!c->rtab_valid) {  // once per context: the reciprocal table, verified exactly
        constexpr int n = erp::kRecipTable;
        if (!ensure(c->rtab, L.rtab.bytes)) return ERP_OUT_OF_MEMORY;
        {  // the magic-number table after it (the sampler's d >= 256 quotients)
            std::vector<uint64_t> mt(n);
            if (!erp::build_magic_table(mt.data(), n)) return ERP_INTERNAL;
            ERP_CK(hipMemcpy(erp::ws_at<uint64_t>(c->rtab.p, L.rtab.magic), mt.data(),
                             (size_t)n * 8, hipMemcpyHostToDevice));
        }
        int32_t* d_bad = erp::ws_at<int32_t>(c->rtab.p, L.rtab.bad);
        ERP_CK(hipMemset(d_bad, 0, 4));
        ERP_CK(erp::launch_recip_table(n, erp::ws_at<double>(c->rtab.p, L.rtab.recip), d_bad,
                                       nullptr));
        int32_t bad = 0;
        ERP_CK(hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost));
        if (bad) return ERP_INTERNAL;
        c->rtab_valid = true;
    }
    return ERP_OK;
}

erp_status upload_w0(erp_ctx* c, const erp_ransac_cfg* cfg, hipStream_t st) {
    if (!c->w0_valid || c->w0_seed != cfg->seed || c->w0_offset != cfg->offset) {
        uint32_t w[31];
        host_glibc_window(cfg->seed, cfg->offset, w);
        ERP_CK(hipMemcpyAsync(c->w0.p, w, sizeof(w), hipMemcpyHostToDevice, st));
        ERP_CK(hipStreamSynchronize(st));
        c->w0_valid = true;
        c->w0_seed = cfg->seed;
        c->w0_offset = cfg->offset;
    }
    return ERP_OK;
}

// a consuming call's preparation, before anything is enqueued or captured: no Philox on a
// stream, the per-pair windows' buffer, the state on the context's device
erp_status stream_prepare(erp_ctx* c, const erp_ransac_cfg* cfg, size_t n_pairs) {
    if (cfg->sampler != ERP_SAMPLER_GLIBC) return ERP_INVALID_ARG;
    if (!ensure(c->w0s, n_pairs * 31 * 4) || !erp::stream_tables_ready())
        return ERP_OUT_OF_MEMORY;
    return erp::rs_to_device(c->rs, c->device);
}

// the consuming launch (counts[P] final): every pair's start window, the state advanced.  The
// stream's event is recorded right here, not at the end of the call, so that calls on other
// contexts that share the stream wait for these two kernels only.
erp_status stream_assign(erp_ctx* c, const erp::BatchShape& sh, const erp_ransac_cfg* cfg,
                         hipStream_t st) {
    erp_rand_stream* s = c->rs;
    StageTimer _t(c, ERP_STAGE_JUMP_PREP, st);
    if (c->rs_capture) {  // (the graph launch takes the stream's turn: erp_pair_batch_run)
        ERP_CK(erp::launch_stream_assign((int32_t*)c->counts.p, sh.n_pairs, cfg->iters,
                                         cfg->sample_frac, s->d_state, (uint32_t*)c->w0s.p, st));
        return ERP_OK;
    }
    RsTurn turn(s, st);
    ERP_CK(erp::launch_stream_assign((int32_t*)c->counts.p, sh.n_pairs, cfg->iters,
                                     cfg->sample_frac, s->d_state, (uint32_t*)c->w0s.p, st));
    return ERP_OK;
}

// the start windows of a call: the stream's per-pair ones, or cfg's (seed, offset) for all
erp_status prepare_w0(erp_ctx* c, const erp_ransac_cfg* cfg, size_t n_pairs, hipStream_t st) {
    return c->rs ? stream_prepare(c, cfg, n_pairs) : upload_w0(c, cfg, st);
}

bool cfg_ok(const erp_ransac_cfg* cfg) {
    return cfg && cfg->iters >= 1 &&
           (cfg->sampler == ERP_SAMPLER_GLIBC || cfg->sampler == ERP_SAMPLER_PHILOX) &&
           cfg->sample_frac > 0 &&
           cfg->sample_frac <= 1.0 && cfg->trim_lo >= 0 && cfg->trim_hi <= 1.0 &&
           cfg->trim_lo <= cfg->trim_hi && cfg->inlier_thr >= 0.0f && cfg->inlier_thr < 1e30f;
}

// caller bearings (erp_initial_guess, erp_eight_point_estimation): every component finite
bool bearings_finite(const double* b, int32_t m) {
    for (size_t k = 0; k < (size_t)m * 3; k++)
        if (!std::isfinite(b[k])) return false;
    return true;
}

// erp_initial_guess's bearing scale (include/erp_match.h).  The Gram pass holds
// the products (l_a l_b)(r_c r_d) 2^44 in six balanced base-256 digits, |product| < 7.97.  With
// c = the largest |component| of one side, that side is multiplied by 2^-e: e = 0 when
// 0.5 <= c <= 1.5 (unit bearings: 0.577 <= c <= 1, so they reach the device byte for byte),
// otherwise the e with 0.5 <= c 2^-e < 1.  Both sides then have c <= 1.5 and every product is
// below 1.5^4 = 5.07.  A power of two is exact and scales the Gram by a power of two: the solved
// vector, R and T are those of the caller's bearings.  c == 0 (no rows, or all zero): e = 0.
int bearing_side_exponent(const double* b, int32_t m) {
    double c = 0.0;
    for (size_t k = 0; k < (size_t)m * 3; k++) c = std::max(c, std::fabs(b[k]));
    if (c == 0.0 || (c >= 0.5 && c <= 1.5)) return 0;
    int e = 0;
    std::frexp(c, &e);  // c = f 2^e, 0.5 <= f < 1
    return e;
}

// the Philox sampler's per-lane LDS bitmap holds M <= 20480 positions (kernels.hip
// launch_philox_sampler); entry points that know m on the host refuse larger pairs up front (the
// batch pipeline, where M is only known on the device, flags the pair instead)
constexpr int32_t kPhiloxMaxM = 20480;
bool sampler_m_ok(const erp_ransac_cfg* cfg, int32_t m) {
    return cfg->sampler != ERP_SAMPLER_PHILOX || m <= kPhiloxMaxM;
}

// the records' E: written when the caller asked for the records or the inlier count reads it
bool want_e(const erp_ransac_cfg* cfg, const erp_batch_outputs* out) {
    return !ERP_SKIP_E || (out && out->hyps) || cfg->inlier_thr > 0.0f;
}

// the opt-in inlier count after the estimate (cfg->inlier_thr > 0; nothing runs otherwise)
erp_status run_inliers(erp_ctx* c, const erp::BatchShape& sh, const erp_ransac_cfg* cfg,
                       erp_hypothesis* hyps, hipStream_t st) {
    if (!(cfg->inlier_thr > 0.0f)) return ERP_OK;
    if (!ensure(c->inl, erp::inlier_scratch_bytes(sh))) return ERP_OUT_OF_MEMORY;
    StageTimer _t(c, ERP_STAGE_INLIERS, st);
    ERP_CK(erp::launch_inliers((int32_t*)c->counts.p, (double*)c->pts.p, sh, cfg->sample_frac,
                               cfg->inlier_thr, c->inl.p, hyps, st));
    return ERP_OK;
}

// the lite estimates (launch_eigen's hl: R1, R2, T as f32 SoA + per-wave counts, no records)
// when nothing reads the records: the caller did not ask for them, the opt-in inlier count is
// off (it adds into the records) and the estimate is not fused into the Gram kernel
bool use_lite(const erp_ransac_cfg* cfg, const erp_batch_outputs* out) {
    return !(out && out->hyps) && !(cfg->inlier_thr > 0.0f) && ERP_FUSE_EIGEN != 2;
}
// whether a launch shares replays (run_hypotheses below says why and when): the pairs' selection
// words then belong to pair rep[p] (c->rep)
bool share_replays(const erp_ctx* c, const erp::BatchShape& sh, bool on_stream) {
    return c->opt[ERP_OPT_SAMPLER_SHARE] != 0 && !on_stream && sh.n_pairs >= 2 &&
           sh.n_pairs <= erp::kAliasMaxPairs;
}
// estimator stages after counts/pts are in place (lite: the estimates in the lite layout)
erp_status run_hypotheses(erp_ctx* c, const erp::BatchShape& sh_in, const erp_ransac_cfg* cfg,
                          const erp_batch_outputs* out, hipStream_t st, bool lite = false,
                          bool on_stream = false) {
    erp_ctx* ctx = c;
    erp::BatchShape sh = sh_in;  // + the sampler / Gram route options
    // the glibc start windows: one per pair from the rand stream (stream_assign), or cfg's
    const uint32_t* w0 = (const uint32_t*)(on_stream ? c->w0s.p : c->w0.p);
    sh.w0_stride = on_stream ? 31 : 0;
    sh.sampler_lat = c->opt[ERP_OPT_SAMPLER_LAT];
    sh.sampler_split = c->opt[ERP_OPT_SAMPLER_SPLIT];
    sh.gram_tiles = c->opt[ERP_OPT_GRAM_TILES];
    sh.sampler_tiers = c->opt[ERP_OPT_SAMPLER_TIERS];
    auto* counts = (int32_t*)c->counts.p;
    auto* flags = (int32_t*)c->flags.p;
    // Shared replays (ERP_OPT_SAMPLER_SHARE, kernels.hip sampler_alias_kernel): with one start
    // window for every pair, and with Philox, a pair's selection words depend on its match count
    // alone, so pairs of this launch with equal counts share the first one's.  Not on a rand
    // stream (every pair has its own window), not for one pair, not above the table's pair
    // limit.  Built on the stream from the device's counts (no sync), whatever stage groups the
    // debug mask leaves on: the table is as cheap as deciding who needs it.
    if (share_replays(c, sh, on_stream)) {
        StageTimer _t(ctx, ERP_STAGE_JUMP_PREP, st);
        ERP_CK(erp::launch_sampler_alias(counts, sh, cfg->sample_frac, (int32_t*)c->rep.p, st));
        sh.rep = (const int32_t*)c->rep.p;
    }
    auto* hyps = (out && out->hyps) ? out->hyps : (erp_hypothesis*)c->hyps.p;
    const erp::ConsensusLayout L = erp::consensus_layout(sh.n_pairs, sh.iters);
    if (cfg->sampler == ERP_SAMPLER_PHILOX) {  // counter-based: no jump polynomials / windows
        if (c->opt[ERP_OPT_DEBUG_STAGES] & 4) {
            StageTimer _t(ctx, ERP_STAGE_SAMPLER, st);
            ERP_CK(erp::launch_philox_sampler(counts, sh, cfg->sample_frac, cfg->seed, cfg->offset,
                                              sh.max_nq, (uint32_t*)c->idx.p, flags, st));
        }
    } else {
        const double* rtab = erp::ws_at<double>(c->rtab.p, L.rtab.recip);
        if (c->opt[ERP_OPT_DEBUG_STAGES] & 2) {
            StageTimer _t(ctx, ERP_STAGE_JUMP_PREP, st);
            ERP_CK(erp::launch_jump_prep(counts, sh, (uint32_t*)c->polyR.p, (uint32_t*)c->polyQ.p,
                                         st));
        }
        if (c->opt[ERP_OPT_DEBUG_STAGES] & 2) {
            StageTimer _t(ctx, ERP_STAGE_WINDOWS, st);
            ERP_CK(erp::launch_sampler(counts, (uint32_t*)c->polyR.p, (uint32_t*)c->polyQ.p,
                                       w0, sh, cfg->sample_frac, rtab,
                                       (uint32_t*)c->wins.p, (uint32_t*)c->idx.p, flags, st, 0));
        }
        if (c->opt[ERP_OPT_DEBUG_STAGES] & 4) {
            StageTimer _t(ctx, ERP_STAGE_SAMPLER, st);
            ERP_CK(erp::launch_sampler(counts, (uint32_t*)c->polyR.p, (uint32_t*)c->polyQ.p,
                                       w0, sh, cfg->sample_frac, rtab,
                                       (uint32_t*)c->wins.p, (uint32_t*)c->idx.p, flags, st, 1));
        }
    }
    if (c->opt[ERP_OPT_DEBUG_STAGES] & 8) {
        StageTimer _t(ctx, ERP_STAGE_GRAM, st);
        ERP_CK(erp::launch_gram_mfma(counts, (double*)c->pts.p, (uint32_t*)c->idx.p, sh,
                                     cfg->sample_frac, (int8_t*)c->limbs.p, (double*)c->gram.p,
                                     out ? out->samples : nullptr,
                                     ERP_FUSE_EIGEN ? (double*)c->gfin.p : nullptr,
                                     ERP_FUSE_EIGEN == 2 ? hyps : nullptr, cfg->valid_abs, st,
                                     flags));
    }
    if (c->opt[ERP_OPT_DEBUG_STAGES] & 32) {
        StageTimer _t(ctx, ERP_STAGE_EIGEN, st);
        ERP_CK(erp::launch_eigen(counts, (double*)c->gram.p, sh, cfg->sample_frac,
                                 cfg->valid_abs, (double*)c->gfin.p, hyps, st, ERP_FUSE_EIGEN,
                                 want_e(cfg, out),
                                 lite ? erp::ws_at<float>(c->hlite.p, L.hlite.hl) : nullptr,
                                 lite ? erp::ws_at<int32_t>(c->hlite.p, L.hlite.wsum) : nullptr));
    }
    return run_inliers(c, sh, cfg, hyps, st);
}

// The pruning refinements of rounds 3-4 (second stage, gradient references, flat route, hinted
// refine windows) were tuned on 128-pair launches.  A launch of a few pairs with a large K
// (configs[4]: one find of 100k iterations, K ~ 89k) runs their per-pair passes on a handful of
// blocks each: there they cost more than they save -- bench.py --workload manual, one box
// (profiles/r06h_manual_opts.txt): 2.11 ms per find with all four, 1.53 ms without.  So their
// automatic setting (-1) is on for launches of >= kFewPairs pairs and off below; an explicit
// option value always wins.  (Results are identical either way: tests/test_gpu_parity.py.)
constexpr int kFewPairs = 8;
struct PruningOpts {
    int lip2, lipg, flat_pct, hint;
};
PruningOpts pruning_opts(const erp_ctx* c, const erp::BatchShape& sh) {
    const bool few = sh.n_pairs < kFewPairs;
    auto pick = [&](int v, int on) { return v >= 0 ? v : (few ? 0 : on); };
    return PruningOpts{pick(c->opt[ERP_OPT_LIP2], 1), pick(c->opt[ERP_OPT_LIPG], 1),
                       pick(c->opt[ERP_OPT_FLAT_REFS], 25), pick(c->opt[ERP_OPT_REFINE_HINT], 1)};
}

// consensus stages after the hypothesis records are in place (counts may be null when the
// valid list is given directly: erp_consensus_dev)
struct ConsensusCall {
    // 0 = everything; 1 = compaction + bounds of rows shard / nshards only (into lb / ub /
    // bsel); 2 = the rest (select onward) after a phase-1 call on this context, with the bounds
    // of every row in lb / ub / bsel (combined over the shards by the caller)
    int phase = 0;
    int shard = 0, nshards = 1;
    double* lb = nullptr;     // the caller's bounds buffers (null: the context's)
    double* ub = nullptr;
    int32_t* bsel = nullptr;
    bool lite = false;        // the estimates are in the lite layout (use_lite)
};
erp_status run_consensus(erp_ctx* c, const erp::BatchShape& sh, const erp_ransac_cfg* cfg,
                         const erp_batch_outputs* out, erp_pair_result* results, hipStream_t st,
                         bool from_hyps, const ConsensusCall& cc = ConsensusCall()) {
    erp_ctx* ctx = c;
    const int phase = cc.phase, shard = cc.shard, nshards = cc.nshards;
    const bool lite = cc.lite;
    erp::ConsensusBufs cb{};
    cb.counts = from_hyps ? (int32_t*)c->counts.p : nullptr;
    cb.flags = (int32_t*)c->flags.p;  // consensus-only: set by consensus_input (non-finite)
    cb.kcount = (int32_t*)c->kcount.p;
    cb.rv = (float*)c->rv.p;
    cb.tv = (out && out->tvec) ? out->tvec : (float*)c->tv.p;
    cb.rv_aos = out ? out->rvec : nullptr;
    cb.dscale = (float*)c->dscale.p;
    cb.tmean = (out && out->dist) ? out->dist : (double*)c->tmean.p;
    cb.lb = cc.lb ? cc.lb : (double*)c->lb.p;
    cb.ub = cc.ub ? cc.ub : (double*)c->ub.p;
    cb.bsel = cc.bsel ? cc.bsel : (int32_t*)c->bsel.p;
    cb.zsel = c->zsel.p;
    cb.surv = c->surv.p;
    cb.nsurv = c->nsurv.p;
    cb.edges = c->edges.p;
    cb.lipref = c->lipref.p;
    cb.sortbuf = c->sortbuf.p;
    cb.hlite = c->hlite.p;
    cb.results = results;
    auto* hyps = (out && out->hyps) ? out->hyps : (erp_hypothesis*)c->hyps.p;
    // small batches (the single-pair call of src/automatic.cpp:117-126): every row gets its
    // K-column histogram, no Lipschitz pre-pruning, no zoom or refine stage.  For one pair at
    // 10k iterations that pass is ~25-35 us of the whole GPU, against ~20 dependent small
    // launches (~0.2 ms) of the pruning stages, which only pay when many pairs share the chip
    // or K is large: the route is taken when n_pairs (2 iters)^2 <= 2e9 (one pair up to ~22k
    // iterations, five at 10k; configs[4]'s 100k-iteration find keeps the pruning), and never
    // for the row-sharded phases.  ERP_OPT_SMALL_BATCH = n >= 0 overrides: batches of <= n pairs
    // take it (0 = never)
    const int sb = c->opt[ERP_OPT_SMALL_BATCH];
    const double kk = 2.0 * sh.iters;
    const bool small = phase == 0 && nshards == 1 &&
                       (sb >= 0 ? sh.n_pairs <= sb : sh.n_pairs * kk * kk <= 2e9);
    const bool prune = !small;
    const PruningOpts po = pruning_opts(c, sh);
    const erp::ConsensusParams cp{cfg->sample_frac, cfg->trim_lo, cfg->trim_hi, shard, nshards,
                                  prune, po.lip2, po.lipg, po.flat_pct, po.hint,
                                  from_hyps && lite};  // (valid_place wrote the edges)
    if (from_hyps && phase != 2 && lite) {
        StageTimer _t(ctx, ERP_STAGE_VALID_COMPACT, st);
        ERP_CK(erp::launch_valid_place(cb, sh, cp, st));
    } else if (from_hyps && phase != 2) {
        StageTimer _t(ctx, ERP_STAGE_VALID_COMPACT, st);
        ERP_CK(erp::launch_valid_compact(cb.counts, hyps, sh, cfg->sample_frac,
                                         (int32_t*)c->vchunk.p, cb.rv, cb.tv, cb.kcount,
                                         cb.rv_aos, cb.dscale, st));
    }
    if (phase != 2) {
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_BOUNDS, st);
        ERP_CK(erp::launch_consensus_bounds(cb, sh, cp, st));
    }
    if (c->opt[ERP_OPT_DEBUG_SNAP] && phase == 0) {
        c->snap_bytes = erp::consensus_snapshot_bytes(sh);
        if (!ensure(c->snap, c->snap_bytes)) return ERP_OUT_OF_MEMORY;
        ERP_CK(erp::consensus_snapshot(cb, sh, cp, c->snap.p, st));
    }
    if (phase == 1) return ERP_OK;
    if (phase == 2)  // the bounds ran per shard (binned rows not combined): report -1
        ERP_CK(erp::consensus_mark_unbinned(cb, sh, st));
    {
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_SELECT, st);
        ERP_CK(erp::launch_consensus_select(cb, sh, cp, 0, st));
    }
    // small batches skip the zoom too: the exact pass takes the first selection's survivors
    // (~150 for a typical pair, one grid-wide launch); single pair 0.487 -> 0.437 ms
    // (profiles/r05g_latency_ab.txt; ERP_OPT_SMALL_ZOOM = 1 keeps it)
    const int zoom_levels = prune || c->opt[ERP_OPT_SMALL_ZOOM] ? c->opt[ERP_OPT_ZOOM_LEVELS] : 0;
    for (int level = 1; level <= zoom_levels; level++) {
        {
            StageTimer _t(ctx, ERP_STAGE_CONSENSUS_BOUNDS, st);
            ERP_CK(erp::launch_consensus_zoom(cb, sh, cp, level, st));
        }
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_SELECT, st);
        ERP_CK(erp::launch_consensus_select(cb, sh, cp, 0, st));
    }
    // (small batches: no refine stage either -- the exact pass takes the survivors in one
    // grid-wide launch; the refine stage's ~8 dependent launches cost a single pair more)
    if (prune) {
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_REFINE, st);
        ERP_CK(erp::launch_consensus_refine(cb, sh, cp, st));
    }
    if (prune) {
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_SELECT, st);
        ERP_CK(erp::launch_consensus_select(cb, sh, cp, 1, st));
    }
    {
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_ROWS, st);
        ERP_CK(erp::launch_consensus_rows(cb, sh, cp, st));
    }
    {
        StageTimer _t(ctx, ERP_STAGE_CONSENSUS_FINAL, st);
        ERP_CK(erp::launch_consensus_final(cb, sh, cp, st));
    }
    if (c->opt[ERP_OPT_DEBUG_SNAP] && phase == 0 && c->snap_bytes) {
        // + the consensus's rotation vectors (SoA [P][3][2 iters] f32) as they are at its end
        const size_t rvb = (size_t)sh.n_pairs * 6 * sh.iters * 4;
        const size_t head = c->snap_bytes;
        DevBuf keep = c->snap;
        if (c->snap.n < head + rvb) {
            c->snap = DevBuf();
            if (!ensure(c->snap, head + rvb)) return ERP_OUT_OF_MEMORY;
            ERP_CK(hipMemcpyAsync(c->snap.p, keep.p, head, hipMemcpyDeviceToDevice, st));
            ERP_CK(hipStreamSynchronize(st));
            free_buf(keep);
        }
        ERP_CK(hipMemcpyAsync((char*)c->snap.p + head, c->rv.p, rvb, hipMemcpyDeviceToDevice, st));
        c->snap_bytes = head + rvb;
    }
    return ERP_OK;
}


erp_status run_estimator(erp_ctx* c, const erp::BatchShape& sh, const erp_ransac_cfg* cfg,
                         const erp_batch_outputs* out, erp_pair_result* results, hipStream_t st) {
    const bool lite = use_lite(cfg, out);
    // (every caller is a consuming entry point: include/erp_match.h "rand stream")
    erp_status es = c->rs ? stream_assign(c, sh, cfg, st) : ERP_OK;
    if (es != ERP_OK) return es;
    es = run_hypotheses(c, sh, cfg, out, st, lite, c->rs != nullptr);
    if (es != ERP_OK) return es;
    if (!(c->opt[ERP_OPT_DEBUG_STAGES] & 16)) return ERP_OK;
    ConsensusCall cc;
    cc.lite = lite;
    return run_consensus(c, sh, cfg, out, results, st, true, cc);
}

// The winner stage behind run_estimator (winner.hip; include/erp_match.h "winner records"): one
// launch over what the run left in the scratch.  Nothing between the estimate and the end of
// run_consensus writes what it reads: the consensus takes counts, flags and hlite (hl, wsum) as
// inputs only (launch_valid_place reads them into rv / tv), and idx, pts and rep are not among
// its buffers at all (ConsensusBufs).  The callers refuse a partial ERP_OPT_DEBUG_STAGES mask,
// which would leave another call's scratch in place.
erp_status run_winners(erp_ctx* c, const erp::BatchShape& sh, const erp_ransac_cfg* cfg,
                       const erp_batch_outputs* out, const erp_pair_result* results,
                       erp_winner* winners, hipStream_t st) {
    const bool lite = use_lite(cfg, out);
    const erp::ConsensusLayout L = erp::consensus_layout(sh.n_pairs, sh.iters);
    erp::WinnerArgs a{};
    a.results = results;
    if (lite) {
        a.hl = erp::ws_at<float>(c->hlite.p, L.hlite.hl);
        a.wsum = erp::ws_at<int32_t>(c->hlite.p, L.hlite.wsum);
    } else {
        a.hyps = (out && out->hyps) ? out->hyps : (const erp_hypothesis*)c->hyps.p;
    }
    a.counts = (const int32_t*)c->counts.p;
    a.pts = (const double*)c->pts.p;
    a.selw = (const uint32_t*)c->idx.p;
    a.rep = share_replays(c, sh, c->rs != nullptr) ? (const int32_t*)c->rep.p : nullptr;
    a.iters = sh.iters;
    a.nwaves = (sh.iters + 63) / 64;
    a.nbw = sh.sel_words;
    a.max_nq = sh.max_nq;
    a.sample_frac = cfg->sample_frac;
    a.valid_abs = cfg->valid_abs;
    a.out = winners;
    ERP_CK(erp::launch_winner(a, sh.n_pairs, st));
    return ERP_OK;
}

// The support stage behind run_estimator (support.hip; include/erp_match.h "support-scored
// winner"): four launches over what the run left in the scratch.  As for run_winners, nothing
// between the estimate and the end of run_consensus writes what it reads.  Checked in
// run_consensus and ConsensusBufs: counts, flags and hlite are the consensus' inputs only
// (launch_valid_place / launch_valid_compact read hl / the records into rv, tv); gfin (the lite
// route's evec), gram and pts are not among ConsensusBufs' buffers, and no launch_consensus_*
// takes them.  So evec, gram, hl, wsum, counts and pts hold at the end of the consensus what the
// estimate read and wrote.  (On the lite route gram holds a pair's Grams only where the fused
// Gram kernel stored them: pairs with s < 9 and the lanes whose evec[0] is NaN -- exactly where
// the prep reads it.)  The callers refuse a partial ERP_OPT_DEBUG_STAGES mask.
struct SupportCall {
    float thr = 0.0f;
    const erp_support_outputs* out = nullptr;
};
bool support_args_ok(const SupportCall& sc) {
    return sc.out && sc.out->support && sc.thr > 0.0f && std::isfinite(sc.thr);
}
erp_status run_support(erp_ctx* c, const erp::BatchShape& sh, const erp_ransac_cfg* cfg,
                       const erp_batch_outputs* out, const erp_pair_result* results,
                       const SupportCall& sc, hipStream_t st) {
    const bool lite = use_lite(cfg, out);
    const erp::ConsensusLayout L = erp::consensus_layout(sh.n_pairs, sh.iters);
    const erp::SupportScratch ss = erp::support_scratch(sh);
    char* eb = erp::ctx_scratch<char>(c, erp::kSlotSupportE,
                                      ss.ec64_bytes + ss.eimg_bytes + ss.xflag_bytes);
    void* ub = erp::ctx_scratch<char>(c, erp::kSlotSupportU, ss.uimg_bytes);
    int32_t* counts = sc.out->counts;
    if (!counts) counts = erp::ctx_scratch<int32_t>(c, erp::kSlotSupportCounts, ss.counts_bytes);
    if (!eb || !ub || !counts) return ERP_OUT_OF_MEMORY;
    erp::SupportArgs a{};
    a.results = results;
    if (lite) {
        a.evec = (const double*)c->gfin.p;
        a.gram = (const double*)c->gram.p;
        a.hl = erp::ws_at<float>(c->hlite.p, L.hlite.hl);
    } else {
        a.hyps = (out && out->hyps) ? out->hyps : (const erp_hypothesis*)c->hyps.p;
    }
    a.mcount = (const int32_t*)c->counts.p;
    a.pts = (const double*)c->pts.p;
    a.iters = sh.iters;
    a.ipad = ss.ipad;
    a.max_nq = sh.max_nq;
    a.mpad = ss.mpad;
    a.mfma = c->opt[ERP_OPT_SUPPORT_COUNT] != 0;
    a.sample_frac = cfg->sample_frac;
    a.valid_abs = cfg->valid_abs;
    a.thr = (double)sc.thr;
    erp::support_band(a.thr, a.mfma != 0, &a.thr_lo, &a.thr_hi);
    a.ec64 = (double*)eb;
    a.eimg = eb + ss.ec64_bytes;
    a.xflag = (int32_t*)(eb + ss.ec64_bytes + ss.eimg_bytes);
    a.uimg = ub;
    a.counts = counts;
    a.support = sc.out->support;
    a.winners = sc.out->winners;
    a.out_results = sc.out->results;
    ERP_CK(erp::launch_support(a, sh.n_pairs, st));
    return ERP_OK;
}

}  // namespace

extern "C" {

erp_status erp_ctx_set_profiling(erp_ctx* ctx, int32_t enable) {
    if (!ctx) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->profiling = enable != 0;
    return ERP_OK;
}

erp_status erp_ctx_set_matcher(erp_ctx* ctx, int32_t method) {
    if (!ctx) return ERP_INVALID_ARG;
    if (method != ERP_MATCHER_MFMA_FILTER && method != ERP_MATCHER_VALU_EXACT)
        return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->matcher = method;
    return ERP_OK;
}

const char* erp_stage_name(int32_t stage) {
    static const char* names[ERP_STAGE_COUNT] = {
        "knn2_filter", "knn2_merge", "bearings", "jump_prep", "sampler",
        "eigen", "valid_compact", "consensus_rows", "consensus_final", "consensus_bounds",
        "consensus_select", "windows", "gram", "knn2_candidates", "knn2_rescore",
        "consensus_refine", "knn2_exact", "sampler_gram", "inliers"};
    return (stage >= 0 && stage < ERP_STAGE_COUNT) ? names[stage] : "unknown";
}

erp_status erp_ctx_stage_times(erp_ctx* ctx, double* total_ms, int64_t* launches) {
    if (!ctx || !total_ms || !launches) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    for (int k = 0; k < ERP_STAGE_COUNT; k++) {
        total_ms[k] = 0;
        launches[k] = 0;
    }
    for (const auto& r : ctx->ev_rec) {
        ERP_CK(hipEventSynchronize(ctx->ev_pool[r.second + 1]));
        float ms = 0;
        ERP_CK(hipEventElapsedTime(&ms, ctx->ev_pool[r.second], ctx->ev_pool[r.second + 1]));
        total_ms[r.first] += ms;
        launches[r.first] += 1;
    }
    ctx->ev_rec.clear();
    ctx->ev_used = 0;
    return ERP_OK;
}

erp_status erp_ctx_reserve(erp_ctx* ctx, int32_t n_pairs, int32_t max_nq, int32_t max_nt,
                           int32_t iters) {
    if (!ctx || n_pairs < 1 || max_nq < 0 || max_nt < 0 || iters < 1) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    const erp::BatchShape sh = make_shape(n_pairs, max_nq, max_nt, iters, 0.25);
    if (!ensure_matcher(ctx, sh) ||
        !ensure(ctx->matches, (size_t)n_pairs * sh.max_nq * sizeof(erp_dmatch)))
        return ERP_OUT_OF_MEMORY;
    return ensure_estimator(ctx, sh, nullptr);
}

}  // extern "C"

namespace {

// the enqueue part of erp_pair_batch_run (every allocation and host upload done before it)
erp_status batch_enqueue(erp_ctx* ctx, const erp_pair_batch* b, float ratio,
                         const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                         const erp::BatchShape& sh, erp_dmatch* matches, hipStream_t st) {
    if (!(ctx->opt[ERP_OPT_DEBUG_STAGES] & 1)) return run_estimator(ctx, sh, cfg, out, out->results, st);
    // the optional outputs read zero past each pair's M / K / s, call after call (a HIP-graph
    // replay or a reused buffer would otherwise keep an earlier call's entries there)
    const size_t P = (size_t)sh.n_pairs, I = (size_t)sh.iters, Q = (size_t)b->max_nq;
    const size_t smax = (size_t)std::max((int)(Q * cfg->sample_frac), 1);
    const struct {
        void* p;
        size_t bytes;
    } opt[] = {{out->matches, P * Q * sizeof(erp_dmatch)}, {out->key_left, P * Q * 8},
               {out->key_right, P * Q * 8}, {out->hyps, P * I * sizeof(erp_hypothesis)},
               {out->samples, P * I * smax * 4}, {out->rvec, P * 2 * I * 12},
               {out->tvec, P * 2 * I * 12}, {out->dist, P * 2 * I * 8}};
    for (const auto& o : opt)
        if (o.p) ERP_CK(hipMemsetAsync(o.p, 0, o.bytes, st));
    if (ctx->matcher == ERP_MATCHER_VALU_EXACT)  // (knn2_split_kernel resets them on the MFMA path)
        ERP_CK(hipMemsetAsync(ctx->flags.p, 0, (size_t)sh.n_pairs * 4, st));
    // the merge writes the gather + bearings as it places each match (src/spherical_surf.cpp:
    // 155-162, src/eight_point.cpp:163-186; bearings_from_matches_kernel's work)
    const erp::BearingOut bo{b->kp_l, b->kp_r, b->width, b->height, (double*)ctx->pts.p,
                             out->key_left, out->key_right};
    erp_status es = run_matcher(ctx, b->desc_l, b->desc_r, b->off_l, b->off_r, sh, ratio, matches,
                                (int32_t*)ctx->counts.p, (int32_t*)ctx->flags.p, st, &bo);
    if (es != ERP_OK) return es;
    return run_estimator(ctx, sh, cfg, out, out->results, st);
}

template <class T>
void key_put(std::vector<uint8_t>& k, const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    k.insert(k.end(), p, p + sizeof(T));
}

// everything a captured pipeline bakes in: the call's structs and the context's scratch pointers
// and route options
std::vector<uint8_t> graph_key(const erp_ctx* c, const erp_pair_batch* b, float ratio,
                               const erp_ransac_cfg* cfg, const erp_batch_outputs* out) {
    std::vector<uint8_t> k;
    key_put(k, *b);
    key_put(k, *cfg);
    key_put(k, *out);
    key_put(k, ratio);
    key_put(k, c->matcher);
    key_put(k, c->opt);
    key_put(k, c->rs);  // the attached rand stream and its device state
    key_put(k, c->rs ? c->rs->d_state : nullptr);
    for (const CtxBuf& b : kCtxBufs)
        if (b.graph) key_put(k, (c->*b.m).p);
    return k;
}

}  // namespace

extern "C" {

erp_status erp_ctx_set_graphs(erp_ctx* ctx, int32_t enable) {
    if (!ctx) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->use_graphs = enable != 0;
    return ERP_OK;
}

erp_status erp_ctx_set_option(erp_ctx* ctx, int32_t option, int32_t value) {
    if (!ctx || option < 0 || option >= ERP_OPT_COUNT) return ERP_INVALID_ARG;
    int lo = 0, hi = 1;  // the on / off options
    switch (option) {
        case ERP_OPT_SMALL_BATCH: lo = -1; hi = INT32_MAX; break;
        case ERP_OPT_SAMPLER_LAT: lo = -1; hi = 2; break;
        case ERP_OPT_SAMPLER_SPLIT: lo = -1; hi = 1; break;
        case ERP_OPT_GRAM_TILES: lo = 0; hi = 2; break;
        case ERP_OPT_ZOOM_LEVELS: lo = 0; hi = 2; break;
        case ERP_OPT_FLAT_REFS: lo = -1; hi = 100; break;
        case ERP_OPT_LIPG: lo = -1; hi = 3; break;  // bit 0: first stage, bit 1: second stage
        case ERP_OPT_LIP2: lo = -1; hi = 1; break;
        case ERP_OPT_REFINE_HINT: lo = -1; hi = 1; break;
        case ERP_OPT_DEBUG_STAGES: lo = -1; hi = 63; break;
        case ERP_OPT_SAMPLER_TIERS: lo = -1; hi = 4; break;
        case ERP_OPT_SAMPLER_SHARE: lo = -1; hi = 1; break;
        case ERP_OPT_SUPPORT_COUNT: lo = -1; hi = 1; break;
        case ERP_OPT_STEREO_CHUNK_MB: lo = 0; hi = 1 << 20; break;
        default: break;
    }
    if (value < lo || value > hi) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ctx->opt[option] = value;
    return ERP_OK;
}

erp_status erp_ctx_get_option(erp_ctx* ctx, int32_t option, int32_t* value) {
    if (!ctx || !value || option < 0 || option >= ERP_OPT_COUNT) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *value = ctx->opt[option];
    return ERP_OK;
}

void erp_debug_set_alloc_pad(size_t bytes) { g_alloc_pad.store(bytes, std::memory_order_relaxed); }

// erp_pair_batch_run (winners == nullptr, sup == nullptr), erp_pair_batch_run_winners and
// erp_pair_batch_run_support, which append their stage and always enqueue plainly
static erp_status pair_batch_run(erp_ctx* ctx, const erp_pair_batch* b, float ratio,
                                 const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                                 erp_winner* winners, void* stream,
                                 const SupportCall* sup = nullptr) {
    if (!ctx || !b || !out || !out->results || !cfg_ok(cfg)) return ERP_INVALID_ARG;
    if (b->n_pairs < 1 || b->dim != erp::kDim || b->max_nq < 0 || b->max_nt < 0 ||
        b->max_nq > 65535 || !b->desc_l || !b->desc_r || !b->kp_l || !b->kp_r || !b->off_l ||
        !b->off_r || !b->width || !b->height)
        return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    if ((winners || sup) && ctx->opt[ERP_OPT_DEBUG_STAGES] != -1) return ERP_INVALID_ARG;
    const erp::BatchShape sh = make_shape(b->n_pairs, b->max_nq, b->max_nt, cfg->iters,
                                          cfg->sample_frac);
    if (!ensure_matcher(ctx, sh)) return ERP_OUT_OF_MEMORY;
    erp_dmatch* matches = out->matches;
    if (!matches) {
        if (!ensure(ctx->matches, (size_t)sh.n_pairs * sh.max_nq * sizeof(erp_dmatch)))
            return ERP_OUT_OF_MEMORY;
        matches = (erp_dmatch*)ctx->matches.p;
    }
    erp_status es = ensure_estimator(ctx, sh, out);
    if (es != ERP_OK) return es;
    es = prepare_w0(ctx, cfg, (size_t)sh.n_pairs, st);
    if (es != ERP_OK) return es;
    if (cfg->inlier_thr > 0.0f && !ensure(ctx->inl, erp::inlier_scratch_bytes(sh)))
        return ERP_OUT_OF_MEMORY;
    // plain enqueue: graphs off, stage timing on, the NULL stream, the debug snapshot (its
    // buffer growth synchronises), or a stream the caller is capturing already (the enqueue
    // then becomes part of the caller's graph)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr) ERP_CK(hipStreamIsCapturing(st, &cap));
    if (!ctx->use_graphs || ctx->profiling || st == nullptr || ctx->opt[ERP_OPT_DEBUG_SNAP] ||
        cap != hipStreamCaptureStatusNone || winners || sup) {
        // (inside the caller's own capture the stream's event cannot order anything: the
        // caller's graph then owns the order of the calls that share the stream)
        ctx->rs_capture = cap != hipStreamCaptureStatusNone;
        es = batch_enqueue(ctx, b, ratio, cfg, out, sh, matches, st);
        ctx->rs_capture = false;
        if (es == ERP_OK && winners) es = run_winners(ctx, sh, cfg, out, out->results, winners, st);
        if (es == ERP_OK && sup) es = run_support(ctx, sh, cfg, out, out->results, *sup, st);
        return es;
    }
    // graph replay: the same call (structs, buffers, scratch) as a captured one -> one launch.
    // On a rand stream the state and the per-pair windows sit at fixed device addresses, so a
    // replay continues the stream; the whole graph launch is the stream's turn.
    auto launch = [&](hipGraphExec_t exec) -> erp_status {
        if (!ctx->rs) {
            ERP_CK(hipGraphLaunch(exec, st));
            return ERP_OK;
        }
        RsTurn turn(ctx->rs, st);
        ERP_CK(hipGraphLaunch(exec, st));
        return ERP_OK;
    };
    std::vector<uint8_t> key = graph_key(ctx, b, ratio, cfg, out);
    for (auto& g : ctx->graphs)
        if (g.key == key) {
            g.used = ++ctx->graph_clock;
            return launch(g.exec);
        }
    ERP_CK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    ctx->rs_capture = true;
    es = batch_enqueue(ctx, b, ratio, cfg, out, sh, matches, st);
    ctx->rs_capture = false;
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(st, &graph);
    if (es != ERP_OK || ce != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return es != ERP_OK ? es : ERP_HIP_ERROR;
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) return ERP_HIP_ERROR;
    if (ctx->graphs.size() >= 8) {  // drop the least recently used
        auto lru = std::min_element(ctx->graphs.begin(), ctx->graphs.end(),
                                    [](const auto& x, const auto& y) { return x.used < y.used; });
        (void)hipGraphExecDestroy(lru->exec);
        ctx->graphs.erase(lru);
    }
    ctx->graphs.push_back({std::move(key), exec, ++ctx->graph_clock});
    return launch(exec);
}

erp_status erp_pair_batch_run(erp_ctx* ctx, const erp_pair_batch* b, float ratio,
                              const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                              void* stream) {
    return pair_batch_run(ctx, b, ratio, cfg, out, nullptr, stream);
}

erp_status erp_pair_batch_run_winners(erp_ctx* ctx, const erp_pair_batch* b, float ratio,
                                      const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                                      erp_winner* d_winners, void* stream) {
    if (!d_winners) return ERP_INVALID_ARG;
    return pair_batch_run(ctx, b, ratio, cfg, out, d_winners, stream);
}

erp_status erp_pair_batch_run_support(erp_ctx* ctx, const erp_pair_batch* b, float ratio,
                                      const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                                      float thr, const erp_support_outputs* sup, void* stream) {
    const SupportCall sc{thr, sup};
    if (!support_args_ok(sc)) return ERP_INVALID_ARG;
    return pair_batch_run(ctx, b, ratio, cfg, out, nullptr, stream, &sc);
}

erp_status erp_match_knn2_ratio(erp_ctx* ctx, const float* d_query, int32_t nq,
                                const float* d_train, int32_t nt, int32_t dim, float ratio,
                                erp_dmatch* d_out, int32_t* d_count, void* stream) {
    if (!ctx || nq < 0 || nt < 0 || dim != erp::kDim || !d_out || !d_count) return ERP_INVALID_ARG;
    if (nq > 0 && (!d_query || !d_train)) return ERP_INVALID_ARG;
    if (nq > 0 && nt < 2) return ERP_TOO_FEW_POINTS;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    if (nq == 0) {
        ERP_CK(hipMemsetAsync(d_count, 0, 4, st));
        return ERP_OK;
    }
    const erp::BatchShape sh = make_shape(1, nq, nt, 1, 0.25);
    if (!ensure_matcher(ctx, sh) || !ensure(ctx->off, 4 * sizeof(int64_t)) ||
        !ensure(ctx->flags, 16))
        return ERP_OUT_OF_MEMORY;
    ERP_CK(erp::launch_set_i64x4((int64_t*)ctx->off.p, 0, nq, 0, nt, st));
    const int64_t* oq = (const int64_t*)ctx->off.p;
    return run_matcher(ctx, d_query, d_train, oq, oq + 2, sh, ratio, d_out, d_count,
                       (int32_t*)ctx->flags.p, st);
}

erp_status erp_match_two_image(erp_ctx* ctx, const float* h_desc1, int32_t n1, const float* h_desc2,
                               int32_t n2, int32_t dim, erp_dmatch* h_out, int32_t* h_count) {
    if (!ctx || n1 < 0 || n2 < 0 || dim != erp::kDim || !h_out || !h_count) return ERP_INVALID_ARG;
    if (n1 > 0 && (!h_desc1 || !h_desc2)) return ERP_INVALID_ARG;
    if (n1 > 0 && n2 < 2) return ERP_TOO_FEW_POINTS;
    *h_count = 0;
    if (n1 == 0) return ERP_OK;
    // one lock across upload, match and download: the staging buffers are the context's
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    if (!ensure(ctx->in_a, (size_t)n1 * dim * 4) || !ensure(ctx->in_b, (size_t)n2 * dim * 4) ||
        !ensure(ctx->in_c, (size_t)n1 * sizeof(erp_dmatch) + 16))
        return ERP_OUT_OF_MEMORY;
    ERP_CK(hipMemcpy(ctx->in_a.p, h_desc1, (size_t)n1 * dim * 4, hipMemcpyHostToDevice));
    ERP_CK(hipMemcpy(ctx->in_b.p, h_desc2, (size_t)n2 * dim * 4, hipMemcpyHostToDevice));
    int32_t* d_count = (int32_t*)((char*)ctx->in_c.p + (size_t)n1 * sizeof(erp_dmatch));
    erp_status s = erp_match_knn2_ratio(ctx, (const float*)ctx->in_a.p, n1, (const float*)ctx->in_b.p,
                                        n2, dim, 0.3f, (erp_dmatch*)ctx->in_c.p, d_count, nullptr);
    if (s != ERP_OK) return s;
    ERP_CK(hipDeviceSynchronize());
    int32_t m = 0;
    ERP_CK(hipMemcpy(&m, d_count, 4, hipMemcpyDeviceToHost));
    if (m > 0) ERP_CK(hipMemcpy(h_out, ctx->in_c.p, (size_t)m * sizeof(erp_dmatch), hipMemcpyDeviceToHost));
    *h_count = m;
    return ERP_OK;
}

// erp_eight_point_find_dev (d_winner == nullptr, sup == nullptr), erp_eight_point_find_winner_dev
// and erp_eight_point_find_support_dev
static erp_status find_dev(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* d_kl,
                           const erp_point2f* d_kr, int32_t m, const erp_ransac_cfg* cfg,
                           erp_pair_result* d_result, erp_hypothesis* d_hyps,
                           erp_winner* d_winner, void* stream,
                           const SupportCall* sup = nullptr) {
    if (!ctx || W <= 0 || H <= 0 || m < 0 || m > 65535 || !d_result || !cfg_ok(cfg) ||
        !sampler_m_ok(cfg, m))
        return ERP_INVALID_ARG;
    if (m > 0 && (!d_kl || !d_kr)) return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    if ((d_winner || sup) && ctx->opt[ERP_OPT_DEBUG_STAGES] != -1) return ERP_INVALID_ARG;
    const erp::BatchShape sh = make_shape(1, m, m, cfg->iters, cfg->sample_frac);
    erp_batch_outputs out{};
    out.results = d_result;
    out.hyps = d_hyps;
    erp_status es = ensure_estimator(ctx, sh, &out);
    if (es != ERP_OK) return es;
    es = prepare_w0(ctx, cfg, 1, st);
    if (es != ERP_OK) return es;
    ERP_CK(hipMemsetAsync(ctx->flags.p, 0, 4, st));
    ERP_CK(erp::launch_set_i32((int32_t*)ctx->counts.p, m, st));
    {
        StageTimer _t(ctx, ERP_STAGE_BEARINGS, st);
        ERP_CK(erp::launch_bearings_direct(d_kl, d_kr, m, W, H, (double*)ctx->pts.p, st));
    }
    es = run_estimator(ctx, sh, cfg, &out, d_result, st);
    if (es == ERP_OK && d_winner) es = run_winners(ctx, sh, cfg, &out, d_result, d_winner, st);
    if (es == ERP_OK && sup) es = run_support(ctx, sh, cfg, &out, d_result, *sup, st);
    return es;
}

erp_status erp_eight_point_find_dev(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* d_kl,
                                    const erp_point2f* d_kr, int32_t m, const erp_ransac_cfg* cfg,
                                    erp_pair_result* d_result, erp_hypothesis* d_hyps,
                                    void* stream) {
    return find_dev(ctx, W, H, d_kl, d_kr, m, cfg, d_result, d_hyps, nullptr, stream);
}

erp_status erp_eight_point_find_winner_dev(erp_ctx* ctx, int32_t W, int32_t H,
                                           const erp_point2f* d_kl, const erp_point2f* d_kr,
                                           int32_t m, const erp_ransac_cfg* cfg,
                                           erp_pair_result* d_result, erp_hypothesis* d_hyps,
                                           erp_winner* d_winner, void* stream) {
    if (!d_winner) return ERP_INVALID_ARG;
    return find_dev(ctx, W, H, d_kl, d_kr, m, cfg, d_result, d_hyps, d_winner, stream);
}

erp_status erp_eight_point_find_support_dev(erp_ctx* ctx, int32_t W, int32_t H,
                                            const erp_point2f* d_kl, const erp_point2f* d_kr,
                                            int32_t m, const erp_ransac_cfg* cfg,
                                            erp_pair_result* d_result, erp_hypothesis* d_hyps,
                                            float thr, const erp_support_outputs* sup,
                                            void* stream) {
    const SupportCall sc{thr, sup};
    if (!support_args_ok(sc)) return ERP_INVALID_ARG;
    return find_dev(ctx, W, H, d_kl, d_kr, m, cfg, d_result, d_hyps, nullptr, stream, &sc);
}

erp_status erp_eight_point_hypotheses_dev(erp_ctx* ctx, int32_t W, int32_t H,
                                          const erp_point2f* d_kl, const erp_point2f* d_kr,
                                          int32_t m, const erp_ransac_cfg* cfg,
                                          erp_hypothesis* d_hyps, void* stream) {
    if (!ctx || W <= 0 || H <= 0 || m < 0 || m > 65535 || !d_hyps || !cfg_ok(cfg) ||
        !sampler_m_ok(cfg, m))
        return ERP_INVALID_ARG;
    if (m > 0 && (!d_kl || !d_kr)) return ERP_INVALID_ARG;
    if ((int32_t)(m * cfg->sample_frac) < 1) return ERP_TOO_FEW_POINTS;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    const erp::BatchShape sh = make_shape(1, m, m, cfg->iters, cfg->sample_frac);
    erp_batch_outputs out{};
    out.hyps = d_hyps;
    erp_status es = ensure_estimator(ctx, sh, &out);
    if (es != ERP_OK) return es;
    es = upload_w0(ctx, cfg, st);
    if (es != ERP_OK) return es;
    ERP_CK(hipMemsetAsync(ctx->flags.p, 0, 4, st));
    ERP_CK(erp::launch_set_i32((int32_t*)ctx->counts.p, m, st));
    {
        StageTimer _t(ctx, ERP_STAGE_BEARINGS, st);
        ERP_CK(erp::launch_bearings_direct(d_kl, d_kr, m, W, H, (double*)ctx->pts.p, st));
    }
    return run_hypotheses(ctx, sh, cfg, &out, st);
}

erp_status erp_consensus_dev(erp_ctx* ctx, const float* d_rvec, const float* d_tvec, int32_t K,
                             double trim_lo, double trim_hi, erp_pair_result* d_result,
                             void* stream) {
    if (!ctx || K < 0 || !d_result || (K > 0 && (!d_rvec || !d_tvec)) || trim_lo < 0 ||
        trim_hi > 1 || trim_lo > trim_hi)
        return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    erp_ransac_cfg cfg;
    erp_ransac_cfg_default(&cfg);
    cfg.trim_lo = trim_lo;
    cfg.trim_hi = trim_hi;
    cfg.iters = std::max((K + 1) / 2, 1);
    const erp::BatchShape sh = make_shape(1, 1, 1, cfg.iters, cfg.sample_frac);
    erp_status es = ensure_estimator(ctx, sh, nullptr);
    if (es != ERP_OK) return es;
    ERP_CK(erp::launch_consensus_input(d_rvec, d_tvec, K, 2 * sh.iters, (float*)ctx->rv.p,
                                       (float*)ctx->tv.p, (int32_t*)ctx->kcount.p,
                                       (float*)ctx->dscale.p, (int32_t*)ctx->flags.p, st));
    return run_consensus(ctx, sh, &cfg, nullptr, d_result, st, false);
}

// the consensus over one pair's hypothesis records (m matches, n_hyps records): the whole of
// it, one shard's bounds or the finish, as cc says
static erp_status consensus_hyps_call(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                      int32_t n_hyps, const erp_ransac_cfg* cfg,
                                      const ConsensusCall& cc, erp_pair_result* d_result,
                                      void* stream) {
    if (!ctx || m < 0 || m > 65535 || n_hyps < 1 || !d_hyps || !cfg_ok(cfg))
        return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    CtxCall call(ctx, st);
    const erp::BatchShape sh = make_shape(1, std::max(m, 1), std::max(m, 1), n_hyps,
                                          cfg->sample_frac);
    erp_batch_outputs out{};
    out.hyps = const_cast<erp_hypothesis*>(d_hyps);  // read only by the consensus stages
    erp_status es = ensure_estimator(ctx, sh, &out);
    if (es != ERP_OK) return es;
    if (cc.phase == 1) {
        const size_t rows = 2 * (size_t)n_hyps;
        ERP_CK(hipMemsetAsync(cc.lb, 0, rows * 8, st));
        ERP_CK(hipMemsetAsync(cc.ub, 0, rows * 8, st));
        ERP_CK(hipMemsetAsync(cc.bsel, 0, rows * 8, st));
    }
    if (cc.phase != 2) {  // (the finish goes on from the shard calls' counts and flags)
        ERP_CK(hipMemsetAsync(ctx->flags.p, 0, 4, st));
        ERP_CK(erp::launch_set_i32((int32_t*)ctx->counts.p, m, st));
    }
    return run_consensus(ctx, sh, cfg, &out, d_result, st, true, cc);
}

erp_status erp_consensus_hyps_dev(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                  int32_t n_hyps, const erp_ransac_cfg* cfg,
                                  erp_pair_result* d_result, void* stream) {
    if (!d_result) return ERP_INVALID_ARG;
    return consensus_hyps_call(ctx, m, d_hyps, n_hyps, cfg, ConsensusCall(), d_result, stream);
}

erp_status erp_consensus_hyps_shard_dev(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                        int32_t n_hyps, const erp_ransac_cfg* cfg, int32_t shard,
                                        int32_t nshards, double* d_lb, double* d_ub,
                                        int32_t* d_bsel, void* stream) {
    if (nshards < 1 || shard < 0 || shard >= nshards || !d_lb || !d_ub || !d_bsel)
        return ERP_INVALID_ARG;
    ConsensusCall cc;
    cc.phase = 1;
    cc.shard = shard;
    cc.nshards = nshards;
    cc.lb = d_lb;
    cc.ub = d_ub;
    cc.bsel = d_bsel;
    return consensus_hyps_call(ctx, m, d_hyps, n_hyps, cfg, cc, nullptr, stream);
}

erp_status erp_consensus_hyps_finish_dev(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                         int32_t n_hyps, const erp_ransac_cfg* cfg, double* d_lb,
                                         double* d_ub, int32_t* d_bsel, erp_pair_result* d_result,
                                         void* stream) {
    if (!d_lb || !d_ub || !d_bsel || !d_result) return ERP_INVALID_ARG;
    ConsensusCall cc;
    cc.phase = 2;
    cc.lb = d_lb;
    cc.ub = d_ub;
    cc.bsel = d_bsel;
    return consensus_hyps_call(ctx, m, d_hyps, n_hyps, cfg, cc, d_result, stream);
}

// erp_eight_point_find (h_winner == nullptr) and erp_eight_point_find_winner: the winner record
// sits behind the result record in the staging buffer
static erp_status find_host(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* h_kl,
                            const erp_point2f* h_kr, int32_t m, const erp_ransac_cfg* cfg,
                            float R_out[3], float T_out[3], erp_pair_result* h_result,
                            erp_winner* h_winner) {
    if (!ctx || m < 0 || (m > 0 && (!h_kl || !h_kr))) return ERP_INVALID_ARG;
    // one lock across upload, find and download: the staging buffers are the context's
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    if (!ensure(ctx->in_c, sizeof(erp_pair_result) + sizeof(erp_winner))) return ERP_OUT_OF_MEMORY;
    erp_status s = erp::upload_keys(ctx, h_kl, h_kr, m);
    if (s != ERP_OK) return s;
    erp_winner* d_winner = h_winner ? (erp_winner*)((erp_pair_result*)ctx->in_c.p + 1) : nullptr;
    s = find_dev(ctx, W, H, erp::keys_left(ctx), erp::keys_right(ctx), m, cfg,
                 (erp_pair_result*)ctx->in_c.p, nullptr, d_winner, nullptr);
    if (s != ERP_OK) return s;
    erp_pair_result r;
    ERP_CK(hipMemcpy(&r, ctx->in_c.p, sizeof(r), hipMemcpyDeviceToHost));
    if (h_winner) ERP_CK(hipMemcpy(h_winner, d_winner, sizeof(*h_winner), hipMemcpyDeviceToHost));
    if (h_result) *h_result = r;
    if (R_out)
        for (int k = 0; k < 3; k++) R_out[k] = r.R[k];
    if (T_out)
        for (int k = 0; k < 3; k++) T_out[k] = r.T[k];
    return (erp_status)r.status;
}

erp_status erp_eight_point_find(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* h_kl,
                                const erp_point2f* h_kr, int32_t m, const erp_ransac_cfg* cfg,
                                float R_out[3], float T_out[3], erp_pair_result* h_result) {
    return find_host(ctx, W, H, h_kl, h_kr, m, cfg, R_out, T_out, h_result, nullptr);
}

erp_status erp_eight_point_find_winner(erp_ctx* ctx, int32_t W, int32_t H,
                                       const erp_point2f* h_kl, const erp_point2f* h_kr,
                                       int32_t m, const erp_ransac_cfg* cfg, float R_out[3],
                                       float T_out[3], erp_pair_result* h_result,
                                       erp_winner* h_winner) {
    if (!h_winner || !cfg_ok(cfg)) return ERP_INVALID_ARG;
    return find_host(ctx, W, H, h_kl, h_kr, m, cfg, R_out, T_out, h_result, h_winner);
}

erp_status erp_eight_point_find_support(erp_ctx* ctx, int32_t W, int32_t H,
                                        const erp_point2f* h_kl, const erp_point2f* h_kr,
                                        int32_t m, const erp_ransac_cfg* cfg, float thr,
                                        float R_out[3], float T_out[3], erp_pair_result* h_result,
                                        erp_support* h_support, erp_winner* h_winner,
                                        erp_pair_result* h_support_result, int32_t* h_counts) {
    // (the stage's arguments first: a call that fails on them must not consume a rand stream)
    if (!ctx || !h_support || !cfg_ok(cfg) || m < 0 || (m > 0 && (!h_kl || !h_kr)) ||
        !(thr > 0.0f) || !std::isfinite(thr))
        return ERP_INVALID_ARG;
    // one lock across upload, find, the stage and download: the staging buffers are the context's
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    ERP_CK(hipSetDevice(ctx->device));
    const erp::SupportStage L(cfg->iters);
    erp_status s = erp::upload_keys(ctx, h_kl, h_kr, m);
    if (s != ERP_OK) return s;
    char* base = erp::ctx_scratch<char>(ctx, erp::kSlotHostStage, L.bytes);
    if (!base) return ERP_OUT_OF_MEMORY;
    erp_pair_result* d_res = (erp_pair_result*)(base + L.result);
    erp_support_outputs so{};
    so.support = (erp_support*)(base + L.support);
    so.winners = (erp_winner*)(base + L.winner);
    so.results = (erp_pair_result*)(base + L.support_result);
    so.counts = (int32_t*)(base + L.counts);
    const SupportCall sc{thr, &so};
    s = find_dev(ctx, W, H, erp::keys_left(ctx), erp::keys_right(ctx), m, cfg, d_res, nullptr,
                 nullptr, nullptr, &sc);
    if (s != ERP_OK) return s;
    erp_pair_result r, sr;
    ERP_CK(hipMemcpy(&r, d_res, sizeof(r), hipMemcpyDeviceToHost));
    ERP_CK(hipMemcpy(&sr, so.results, sizeof(sr), hipMemcpyDeviceToHost));
    ERP_CK(hipMemcpy(h_support, so.support, sizeof(*h_support), hipMemcpyDeviceToHost));
    if (h_winner) ERP_CK(hipMemcpy(h_winner, so.winners, sizeof(*h_winner), hipMemcpyDeviceToHost));
    if (h_counts)
        ERP_CK(hipMemcpy(h_counts, so.counts, (size_t)cfg->iters * 4, hipMemcpyDeviceToHost));
    if (h_result) *h_result = r;
    if (h_support_result) *h_support_result = sr;
    if (R_out)
        for (int k = 0; k < 3; k++) R_out[k] = sr.R[k];
    if (T_out)
        for (int k = 0; k < 3; k++) T_out[k] = sr.T[k];
    return (erp_status)r.status;
}

erp_status erp_initial_guess(erp_ctx* ctx, const double* h_bl, const double* h_br, int32_t m,
                             const erp_ransac_cfg* cfg, float R_out[3], float T_out[3],
                             erp_pair_result* h_result) {
    if (!ctx || m < 0 || m > 65535 || (m > 0 && (!h_bl || !h_br)) || !cfg_ok(cfg) ||
        !sampler_m_ok(cfg, m))
        return ERP_INVALID_ARG;
    if (!bearings_finite(h_bl, m) || !bearings_finite(h_br, m)) return ERP_INVALID_ARG;
    const int el = bearing_side_exponent(h_bl, m), er = bearing_side_exponent(h_br, m);
    erp_pair_result r;
    {
        ERP_CK(hipSetDevice(ctx->device));
        HostCtxCall call(ctx);
        const erp::BatchShape sh = make_shape(1, m, m, cfg->iters, cfg->sample_frac);
        erp_status es = ensure_estimator(ctx, sh, nullptr);
        if (es != ERP_OK) return es;
        if (!ensure(ctx->in_c, sizeof(erp_pair_result))) return ERP_OUT_OF_MEMORY;
        es = prepare_w0(ctx, cfg, 1, nullptr);
        if (es != ERP_OK) return es;
        std::vector<double> pts((size_t)(m + 1) * 6, 0.0);
        for (int32_t i = 0; i < m; i++)
            for (int k = 0; k < 3; k++) {
                pts[(size_t)i * 6 + k] = std::ldexp(h_bl[(size_t)i * 3 + k], -el);
                pts[(size_t)i * 6 + 3 + k] = std::ldexp(h_br[(size_t)i * 3 + k], -er);
            }
        ERP_CK(hipMemcpy(ctx->pts.p, pts.data(), (size_t)(m + 1) * 48, hipMemcpyHostToDevice));
        ERP_CK(hipMemcpy(ctx->counts.p, &m, 4, hipMemcpyHostToDevice));
        ERP_CK(hipMemset(ctx->flags.p, 0, 4));
        es = run_estimator(ctx, sh, cfg, nullptr, (erp_pair_result*)ctx->in_c.p, nullptr);
        if (es != ERP_OK) return es;
        ERP_CK(hipMemcpy(&r, ctx->in_c.p, sizeof(r), hipMemcpyDeviceToHost));
    }
    if (h_result) *h_result = r;
    if (R_out)
        for (int k = 0; k < 3; k++) R_out[k] = r.R[k];
    if (T_out)
        for (int k = 0; k < 3; k++) T_out[k] = r.T[k];
    return (erp_status)r.status;
}

erp_status erp_eight_point_estimation(erp_ctx* ctx, const double* h_bl, const double* h_br,
                                      int32_t m, erp_hypothesis* h_out) {
    if (!ctx || m < 0 || !h_out || (m > 0 && (!h_bl || !h_br))) return ERP_INVALID_ARG;
    if (m < 1) return ERP_TOO_FEW_POINTS;
    if (!bearings_finite(h_bl, m) || !bearings_finite(h_br, m)) return ERP_INVALID_ARG;
    ERP_CK(hipSetDevice(ctx->device));
    HostCtxCall call(ctx);
    if (!ensure(ctx->in_d, (size_t)m * 48 + 36 * 8 * 2 + sizeof(erp_hypothesis) + 64))
        return ERP_OUT_OF_MEMORY;
    std::vector<double> pts((size_t)m * 6);
    for (int32_t i = 0; i < m; i++)
        for (int k = 0; k < 3; k++) {
            pts[(size_t)i * 6 + k] = h_bl[(size_t)i * 3 + k];
            pts[(size_t)i * 6 + 3 + k] = h_br[(size_t)i * 3 + k];
        }
    char* base = (char*)ctx->in_d.p;
    double* d_pts = (double*)base;
    double* d_gram = (double*)(base + (size_t)m * 48);
    double* d_gfin = (double*)(base + (size_t)m * 48 + 36 * 8);
    int32_t* d_cnt = (int32_t*)(base + (size_t)m * 48 + 36 * 8 * 2);
    erp_hypothesis* d_h = (erp_hypothesis*)(base + (size_t)m * 48 + 36 * 8 * 2 + 16);
    ERP_CK(hipMemcpy(d_pts, pts.data(), pts.size() * 8, hipMemcpyHostToDevice));
    ERP_CK(hipMemcpy(d_cnt, &m, 4, hipMemcpyHostToDevice));
    ERP_CK(erp::launch_gram_all(d_pts, m, d_gram, nullptr));
    erp::BatchShape sh = make_shape(1, m, m, 1, 1.0);
    ERP_CK(erp::launch_eigen(d_cnt, d_gram, sh, 1.0, 1.57, d_gfin, d_h, nullptr));
    ERP_CK(hipMemcpy(h_out, d_h, sizeof(erp_hypothesis), hipMemcpyDeviceToHost));
    return ERP_OK;
}

}  // extern "C"

extern "C" int erp_debug_lip_counters(uint32_t* out64) { return erp::debug_lip_counters(out64); }

// debug (after erp_debug_set_alloc_pad(N), N > 0): buffers whose canary bytes were overwritten,
// reported on stderr; returns their number (0 when no pad is set)
extern "C" int erp_debug_check_pads(void) {
    const size_t pad = alloc_pad();
    if (!pad) return 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::lock_guard<std::mutex> g(g_pad_mu);
    std::vector<unsigned char> h(pad);
    int bad = 0;
    for (auto& e : g_padded) {
        if (hipMemcpy(h.data(), (char*)e.first + e.second, pad, hipMemcpyDeviceToHost) != hipSuccess)
            return -1;
        size_t first = pad, last = 0;
        for (size_t i = 0; i < pad; i++)
            if (h[i] != 0xA5) first = std::min(first, i), last = i;
        if (first < pad) {
            bad++;
            fprintf(stderr, "erp_debug_check_pads: buffer of %zu bytes at %p: canary bytes %zu .. %zu overwritten\n",
                    e.second, e.first, first, last);
        }
    }
    return bad;
}

// debug (context option ERP_OPT_DEBUG_SNAP = 1): the last run's snapshot (lb [P][2 iters] f64,
// ub, first-stage counts [P] i32) into host memory; returns the snapshot's size in bytes (0: none)
extern "C" long long erp_debug_snapshot(erp_ctx* ctx, void* host, size_t bytes) {
    if (!ctx || !ctx->snap_bytes) return 0;
    if (host && bytes >= ctx->snap_bytes) {
        if (hipDeviceSynchronize() != hipSuccess) return -1;
        if (hipMemcpy(host, ctx->snap.p, ctx->snap_bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    return (long long)ctx->snap_bytes;
}

extern "C" {

erp_status erp_ctx_set_rand_stream(erp_ctx* ctx, erp_rand_stream* s) {
    if (!ctx) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (s) {
        std::lock_guard<std::mutex> g(s->mu);
        if (s->device >= 0 && s->device != ctx->device) return ERP_INVALID_ARG;
    }
    ctx->rs = s;
    return ERP_OK;
}

erp_status erp_ctx_get_rand_stream(erp_ctx* ctx, erp_rand_stream** out) {
    if (!ctx || !out) return ERP_INVALID_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = ctx->rs;
    return ERP_OK;
}

}  // extern "C"

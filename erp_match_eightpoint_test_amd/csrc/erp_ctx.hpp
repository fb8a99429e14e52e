// erp_ctx.hpp -- the context every host file of the library works on (private): erp_ctx and
// erp_rand_stream behind include/erp_match.h's opaque pointers, the grow-only device buffers,
// the one table of scratch slots, and the guards of a call (CtxCall), of a stream's turn
// (RsTurn) and of a timed stage (StageTimer).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <utility>
#include <vector>

#include "../../include/erp_match.h"
#include "erp_host_stage.hpp"

#define ERP_CK(x)                                         \
    do {                                                  \
        if ((x) != hipSuccess) return ERP_HIP_ERROR;      \
    } while (0)

namespace erp {

struct DevBuf {
    void* p = nullptr;
    size_t n = 0;
};
// grow-only device buffer; returns false on allocation failure (capi.hip)
bool ensure(DevBuf& b, size_t bytes);
// frees b (and forgets its canary record)
void free_buf(DevBuf& b);

// The context's scratch slots (erp_ctx::extra, handed out by ctx_scratch): one image-batch or
// sweep call uses the remap's, SURF's and its own at the same time, so every user has its own.
enum CtxSlot {
    kSlotRemapList,    // remap_api.hip: the boundary list of a remap launch
    // surf_api.hip: the layer table (erp_ctx::surf_key), the per-image buffers, the descriptor
    // pass's chunk pool / jobs / items and the keypoint prefix
    kSlotSurfLayers, kSlotSurfGray, kSlotSurfSum, kSlotSurfDet, kSlotSurfRaw, kSlotSurfSorted,
    kSlotSurfDesc, kSlotSurfPool, kSlotSurfJobs, kSlotSurfItems, kSlotSurfKpre,
    kSlotVizStamps,    // viz.hip: draw_match's line stamps (erp_ctx::viz_epoch)
    // the group of the batched do_all and of the sweep (image_batch.hip, sweep.hip): band
    // canvases, SURF's padded keypoints / descriptors / counts, the pack step's row bases
    kSlotBands, kSlotKp, kSlotDesc, kSlotCount, kSlotRowBase,
    // sweep.hip: the group's rotated images, the left image's keypoints / descriptors / counts,
    // the matched keypoints of erp_image_sweep_run's match error
    kSlotSweepCanvas, kSlotLeftKp, kSlotLeftDesc, kSlotLeftCount, kSlotSweepKeyL, kSlotSweepKeyR,
    // the device side of erp_eight_point_find_polished, erp_eight_point_find_posed and
    // erp_match_guided, laid out by erp_host_stage.hpp: each call holds the context lock from
    // its upload to its blocking download, so the three never use the slot at the same time
    kSlotHostStage,
    // guided.hip: the per-query (j0, e0, e1, |G_i|) records, the per-train-row 64-bit claim
    // words, and the train bearings with each pair's E'
    kSlotGuidedQuery, kSlotGuidedClaim, kSlotGuidedBearings,
    // support.hip: every iteration's E' (fp64, the count kernel's operand image, the fp64-only
    // flags), the matches' u = l (x) r image, and the counts when the caller keeps none
    kSlotSupportE, kSlotSupportU, kSlotSupportCounts,
    // stereo.hip: a chunk's census words (left then right), its S volume, and its winners
    // (d* then dR)
    kSlotStereoCensus, kSlotStereoVolume, kSlotStereoWinners,
    kCtxSlotCount
};

}  // namespace erp

// A rand stream (include/erp_match.h): host state until the first GPU call that uses it, then
// the device copy d_state (erp_kernels.hpp kStream*) is the authoritative one.
struct erp_rand_stream {
    std::mutex mu;            // calls take the stream in the order they lock it
    uint32_t seed = 1;
    uint64_t draws = 0;
    uint32_t win[31] = {};
    int device = -1;          // the device of d_state (a process stream: fixed from the start)
    uint32_t* d_state = nullptr;
    // recorded right after the last kernel that touched d_state; the next one waits for it
    hipEvent_t ev = nullptr;
    bool pending = false;
    bool process_owned = false;
};

struct erp_ctx {
    using DevBuf = erp::DevBuf;
    int device = 0;
    // one lock per context; recursive so the host-pointer entry points hold it across their
    // copies AND the device entry point they call
    std::recursive_mutex mu;
    // stream ordering between calls (the scratch below is shared by every call): the end of
    // the last call's work, and the stream it was enqueued on
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool pending = false;
    // stage timing
    bool profiling = false;
    int32_t matcher = ERP_MATCHER_MFMA_FILTER;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<int, size_t>> ev_rec;  // (stage, index of start event; end = +1)
    DevBuf mblk;              // knn2_merge's per-block survivor counts
    DevBuf zsel;              // consensus zoom: the survivors' rank-window bins (level 1 grid)
    DevBuf part, part1, pu, ccount, cand, bsel, edges, gfin, matches, counts, flags, pts, polyR, polyQ, idx, gram, hyps, rv, tv, kcount, tmean,
        sortbuf, w0, off, wh, results, in_a, in_b, in_c, in_d, dscale, lb, ub, surv, nsurv, wins,
        rtab, limbs, tsplit, ovf, vchunk, lipref, inl, hlite,
        w0s,                  // per-pair start windows [P][31] of a call on a rand stream
        rep;                  // the launch's alias table [P] (run_hypotheses, shared replays)
    // the attached rand stream (erp_ctx_set_rand_stream; not owned) and whether the current
    // enqueue is being captured into a graph (the stream's event is then handled around the
    // graph launch: an event inside a captured region orders nothing outside it)
    erp_rand_stream* rs = nullptr;
    bool rs_capture = false;
    DevBuf extra[erp::kCtxSlotCount];  // the scratch slots (erp::ctx_scratch)
    // route options (erp_ctx_set_option; include/erp_match.h documents each, defaults below)
    int32_t opt[ERP_OPT_COUNT] = {
        -1,  // SMALL_BATCH: auto
        -1,  // SAMPLER_LAT: auto
        -1,  // SAMPLER_SPLIT: auto
        0,   // GRAM_TILES: auto
        // ZOOM_LEVELS: 0 since r05 -- with the hinted refine windows (r04) the survivors' zoom
        // no longer pays for itself; same-box A/B per 768-pair step (profiles/r05w_ab_zoom.txt):
        // consensus 5.81 / 5.87 -> 5.67 / 5.67 ms, worst-case batch 16.2 / 16.1k -> 16.6 /
        // 16.5k pairs/s.  (The second pre-pruning stage's fine pass uses the zoom kernel either way.)
        0,
        0,   // SMALL_ZOOM: the small-batch route skips the zoom (single pair 0.487 -> 0.437 ms)
        // LIP2 / LIPG / REFINE_HINT / FLAT_REFS: -1 = automatic (pruning_opts): on for batches of
        // >= kFewPairs pairs, off below
        -1,  // LIP2: the second pre-pruning stage (kernels.hip consensus_lipschitz2_kernel)
        -1,  // LIPG: the central references' distance gradient (consensus_grad_kernel)
        -1,  // REFINE_HINT: sub-bins on each row's Lipschitz interval (consensus_hint_kernel)
        -1,  // FLAT_REFS: pairs whose first stage kept > 25 % of the rows take the flat route
        1,   // BOUND_RATIO: the matcher's ratio test from the bf16 bounds where they suffice
        -1,  // DEBUG_STAGES: every stage group
        0,   // DEBUG_SNAP
        -1,  // SAMPLER_TIERS: auto
        1,   // VERTICAL_SHARED: the batched vertical stage's shared-map kernel
        -1,  // SAMPLER_SHARE: pairs of a launch with equal match counts share one replay
        -1,  // SUPPORT_COUNT: the support stage's count on bf16 MFMA (auto) or f32 VALU
        1024};  // STEREO_CHUNK_MB: the S volume a chunk of stereo pairs may take (stereo.hip)
    // debug (ERP_OPT_DEBUG_SNAP): lb, ub and the first-stage list counts right after the bounds
    // pass, fetched with erp_debug_snapshot
    DevBuf snap;
    size_t snap_bytes = 0;
    uint64_t surf_key = 0;    // (W, H, params) of the SURF layer table in kSlotSurfLayers
    uint32_t viz_epoch = 0;   // stamp epoch of the draw_match line buffer (kSlotVizStamps)
    // HIP-graph replay of erp_pair_batch_run (erp_ctx_set_graphs): key bytes -> executable graph
    bool use_graphs = false;
    struct Graph {
        std::vector<uint8_t> key;
        hipGraphExec_t exec = nullptr;
        uint64_t used = 0;
    };
    std::vector<Graph> graphs;
    uint64_t graph_clock = 0;
    bool rtab_valid = false;  // rtab[d] = 1/d rounded up (the sampler's exact modulo)
    bool w0_valid = false;
    uint32_t w0_seed = 0;
    uint64_t w0_offset = 0;
};

// glibc rand() window before draw `offset` of a stream seeded with `seed`: the 31 words
// r[n-31..n-1] (rand_stream.hip)
void host_glibc_window(uint32_t seed, uint64_t offset, uint32_t out[31]);
// iota + std::random_shuffle of m entries on the window `ring`, the first n into h_idx; ring
// ends up m - 1 draws further on (viz.hip)
void erp_shuffle_prefix_window(uint32_t ring[31], int32_t m, int32_t n, int32_t* h_idx);

namespace erp {

// the stream's state into device memory on `device` (once; blocking, so never inside a
// capture); rand_stream.hip
erp_status rs_to_device(erp_rand_stream* s, int device);

// slot's buffer grown to >= bytes (grow-only, under the context lock); nullptr when out of memory
template <class T>
T* ctx_scratch(erp_ctx* ctx, CtxSlot slot, size_t bytes) {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    DevBuf& b = ctx->extra[slot];
    return ensure(b, bytes) ? (T*)b.p : nullptr;
}

// A one-pair host call's keypoints into in_a / in_b (blocking copies, under the context lock).
inline erp_status upload_keys(erp_ctx* ctx, const erp_point2f* h_kl, const erp_point2f* h_kr,
                              int32_t m) {
    if (!ensure(ctx->in_a, (size_t)m * 8 + 8) || !ensure(ctx->in_b, (size_t)m * 8 + 8))
        return ERP_OUT_OF_MEMORY;
    if (m > 0) {
        ERP_CK(hipMemcpy(ctx->in_a.p, h_kl, (size_t)m * 8, hipMemcpyHostToDevice));
        ERP_CK(hipMemcpy(ctx->in_b.p, h_kr, (size_t)m * 8, hipMemcpyHostToDevice));
    }
    return ERP_OK;
}
inline const erp_point2f* keys_left(const erp_ctx* ctx) { return (const erp_point2f*)ctx->in_a.p; }
inline const erp_point2f* keys_right(const erp_ctx* ctx) { return (const erp_point2f*)ctx->in_b.p; }

// the stage inputs of such a call (erp_polish_inputs, erp_pose_inputs: the same leading fields)
// over the uploaded keypoints; d_wh = {W, H} on the device
template <class In>
In one_pair_inputs(const erp_ctx* ctx, int32_t m, const int32_t* d_wh, const erp_pair_result* d_res) {
    In in{};
    in.n_pairs = 1;
    in.key_stride = m;
    in.key_left = keys_left(ctx);
    in.key_right = keys_right(ctx);
    in.width = d_wh;
    in.height = d_wh + 1;
    in.results = d_res;
    return in;
}

// records an event pair around one launch when profiling is on
struct StageTimer {
    erp_ctx* c;
    int stage;
    hipStream_t st;
    size_t idx = (size_t)-1;
    StageTimer(erp_ctx* c_, int stage_, hipStream_t st_) : c(c_), stage(stage_), st(st_) {
        if (!c->profiling) return;
        while (c->ev_pool.size() < c->ev_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            c->ev_pool.push_back(e);
        }
        idx = c->ev_used;
        c->ev_used += 2;
        (void)hipEventRecord(c->ev_pool[idx], st);
    }
    ~StageTimer() {
        if (idx == (size_t)-1) return;
        (void)hipEventRecord(c->ev_pool[idx + 1], st);
        c->ev_rec.emplace_back(stage, idx);
    }
};

// A call's enqueue section on a context: holds the context lock, makes this call's stream wait
// for the previous call's work when that went to another stream (every call shares the
// context's scratch, so two calls on different streams would otherwise race on it), and on
// exit records the end of this call's work.  Calls on one stream stay in stream order for free.
struct CtxCall {
    erp_ctx* c;
    hipStream_t st;
    CtxCall(erp_ctx* c_, hipStream_t st_) : c(c_), st(st_) {
        c->mu.lock();
        if (c->pending && st != c->last) (void)hipStreamWaitEvent(st, c->done, 0);
    }
    ~CtxCall() {
        if (!c->done) (void)hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
        if (c->done && hipEventRecord(c->done, st) == hipSuccess) {
            c->last = st;
            c->pending = true;
        }
        c->mu.unlock();
    }
    CtxCall(const CtxCall&) = delete;
    CtxCall& operator=(const CtxCall&) = delete;
};

// The host-pointer entry points that write the shared scratch with blocking copies (null
// stream): join the context's call order and wait on the host for the previous call's device
// work first -- the null stream does not synchronise with non-blocking streams, so an earlier
// *_dev call on such a stream may still be reading the buffers about to be overwritten.
struct HostCtxCall : CtxCall {
    explicit HostCtxCall(erp_ctx* c_) : CtxCall(c_, nullptr) {
        if (c->pending) (void)hipEventSynchronize(c->done);
    }
};

// a stream's turn on HIP stream st: holds the stream's lock, makes st wait for the last kernel
// that touched the state, and on exit records the end of this turn's kernels
struct RsTurn {
    erp_rand_stream* s;
    hipStream_t st;
    RsTurn(erp_rand_stream* s_, hipStream_t st_) : s(s_), st(st_) {
        s->mu.lock();
        if (s->pending) (void)hipStreamWaitEvent(st, s->ev, 0);
    }
    ~RsTurn() {
        if (hipEventRecord(s->ev, st) == hipSuccess) s->pending = true;
        s->mu.unlock();
    }
    RsTurn(const RsTurn&) = delete;
    RsTurn& operator=(const RsTurn&) = delete;
};

}  // namespace erp

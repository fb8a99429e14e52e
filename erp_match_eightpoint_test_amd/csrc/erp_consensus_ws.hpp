// erp_consensus_ws.hpp -- the one owner of the consensus stage's device scratch layout: for a
// batch of n_pairs pairs at iters iterations, the byte size of every context buffer the stage
// uses and the byte offset / element count of every named part inside it.  Host only, plain
// C++17, no HIP types: the context allocates by it (capi.hip ensure_estimator), the launchers
// get their typed pointers from it (kernels.hip consensus_views), and a stand-alone g++ program
// checks it (tests/cpp/consensus_layout_check.cpp).
// Precondition: every buffer's base address is at least 16-byte aligned (hipMalloc gives 256),
// so an offset's alignment is the address's.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace erp {

// bins of the bounds pass (kernels.hip consensus_bounds_kernel): bin = key >> kBinShift
constexpr int kBinShift = 19;         // 16 bins per binade of s = d^2
constexpr int kMantBits = 23 - kBinShift;
constexpr int kBinsPerBinade = 1 << kMantBits;  // (= 32 per binade of the distance)
constexpr int kBinades = 36;          // of s (576 bins: 4 blocks of 39 KB per CU)
constexpr int kNB = kBinsPerBinade * kBinades;  // 576
#ifndef ERP_LIP2_STEP
#define ERP_LIP2_STEP 4
#endif
constexpr int kLip2Step = ERP_LIP2_STEP;  // 1 in 4 L1 rows is a second-stage reference
constexpr int kHintCands = 4;         // rank-key hint candidates per pair (consensus_hint_kernel)
// rtab[d] = 1/d rounded up, d < kRecipTable (the sampler's exact modulo)
constexpr int kRecipTable = 65538;
// sizes of the two kernel-side types the layout holds (kernels.hip ties them to the real types)
constexpr size_t kFloat4Bytes = 16;
constexpr size_t kHintCandBytes = 24;  // HintCand: f64 T, i32 row, u32 va, vb, pad

struct WsPart {
    size_t off;    // bytes from the buffer's base
    size_t count;  // elements
    size_t elem;   // bytes per element
    size_t align;  // of off (= of the address, by the precondition above)
    constexpr size_t end() const { return off + count * elem; }
};

// a part's typed address in the buffer at base
template <class T>
inline T* ws_at(void* base, const WsPart& p) {
    return reinterpret_cast<T*>(static_cast<char*>(base) + p.off);
}

constexpr size_t ws_align_up(size_t off, size_t a) { return (off + a - 1) / a * a; }

// power of two >= 2 * iters: a pair's row stride in sortbuf's float role
inline int sortbuf_len(int iters) {
    int p = 1;
    while (p < 2 * iters) p <<= 1;
    return p;
}

struct ConsensusLayout {
    size_t P, stride;  // pairs; rows per pair = 2 * iters
    // per-row buffers, no sub-parts: lb / ub [P][stride] f64, bsel / zsel [P][stride][2] i32,
    // surv [P][stride] i32
    size_t lb_bytes, ub_bytes, bsel_bytes, zsel_bytes, surv_bytes;
    struct {  // the context's nsurv buffer: five count arrays
        size_t bytes;
        WsPart nsurv;  // [P] survivors of the last select
        WsPart nbin;   // [P] rows the bounds pass binned (-1: every row)
        WsPart uoff;   // [P + 1] unit prefix of whichever list pass runs next
        WsPart n2;     // [P] counts of list2
        WsPart nfb;    // [P] the second stage's fall-back counts
    } counts;
    struct {
        size_t bytes;
        WsPart first;  // [P][2][kNB] f32 first-pass edges
        WsPart zoom;   // [P][2][kNB] f32 zoom edges
        WsPart zgrid;  // [P] i32 zoom grids
    } edges;
    struct {  // the pruning references' scratch
        size_t bytes;
        size_t cap;      // references per pair, >= those of any mode
        size_t gcap;     // gradient references per pair
        WsPart ref;      // [P][cap] float4 (x, y, z, squared pruning radius)
        WsPart U;        // [P] f64 smallest UB of the references
        WsPart cnt;      // [P] i32
        WsPart r2cnt;    // [P] i32 counts of r2list
        WsPart r2list;   // [P][stride] i32 second-stage reference list
        WsPart gref;     // [P][gcap][2] float4, 64 bytes after r2list, rounded up to 16
        WsPart gsel;     // [P][gcap] i32
        WsPart gcnt;     // [P] i32
        WsPart goff;     // [P + 1] i32
        WsPart nflat;    // [P] i32 flat gate (consensus_flat_gate_kernel)
        WsPart hcand;    // [P][kHintCands] HintCand, rounded up to 16
        size_t snap_bytes;  // the debug snapshot's share: ref, U, cnt (contiguous from 0)
    } lipref;
    struct {  // two roles, never live together: list2 is free until consensus_final scores ties
        size_t bytes;
        WsPart score;  // [P][len] f32 exact tie re-scoring scratch (consensus_final_kernel)
        WsPart list2;  // the same bytes as i32 row lists of the pre-pruning / refine stages
        size_t len;                  // sortbuf_len(iters)
        size_t list2_bounds_stride;  // rows per pair as the bounds stage indexes list2 (stride)
        size_t list2_refine_stride;  // ... and as the refine stage does (len)
    } sortbuf;
    struct {  // the lite estimates (launch_eigen's hl)
        size_t bytes;
        WsPart hl;    // [P][9][iters] f32 R1, R2, T
        WsPart wsum;  // [P][waves of 64 iterations][8] i32 counts / bounding boxes
    } hlite;
    struct {  // the sampler's tables (shape-independent)
        size_t bytes;
        WsPart recip;  // [kRecipTable] f64
        WsPart magic;  // [kRecipTable] u64 (ERP_SAMPLER_MAGIC)
        WsPart bad;    // [1] i32 check counter
    } rtab;
};

inline ConsensusLayout consensus_layout(int n_pairs, int iters) {
    ConsensusLayout l{};
    const size_t P = (size_t)n_pairs, S = 2 * (size_t)iters;
    // consecutive parts: each starts where the one before it ends
    auto after = [](const WsPart& prev, size_t count, size_t elem) {
        return WsPart{prev.end(), count, elem, elem < 16 ? elem : 16};
    };
    l.P = P;
    l.stride = S;
    l.lb_bytes = l.ub_bytes = l.bsel_bytes = l.zsel_bytes = P * S * 8;
    l.surv_bytes = P * S * 4;

    auto& c = l.counts;
    c.nsurv = WsPart{0, P, 4, 4};
    c.nbin = after(c.nsurv, P, 4);
    c.uoff = after(c.nbin, P + 1, 4);
    c.n2 = after(c.uoff, P, 4);
    c.nfb = after(c.n2, P, 4);
    c.bytes = P * 20 + 8;

    auto& e = l.edges;
    e.first = WsPart{0, P * 2 * kNB, 4, 4};
    e.zoom = after(e.first, P * 2 * kNB, 4);
    e.zgrid = after(e.zoom, P, 4);
    e.bytes = e.zgrid.end();

    auto& r = l.lipref;
    r.cap = S / kLip2Step + 64;
    r.gcap = S / 4 + 64;  // >= the stage-1 references; the second stage's are capped at it
    r.ref = WsPart{0, P * r.cap, kFloat4Bytes, 16};
    r.U = after(r.ref, P, 8);
    r.cnt = after(r.U, P, 4);
    r.r2cnt = after(r.cnt, P, 4);
    r.r2list = after(r.r2cnt, P * S, 4);
    r.gref = WsPart{ws_align_up(r.r2list.end() + 64, 16), P * r.gcap * 2, kFloat4Bytes, 16};
    r.gsel = after(r.gref, P * r.gcap, 4);
    r.gcnt = after(r.gsel, P, 4);
    r.goff = after(r.gcnt, P + 1, 4);
    r.nflat = after(r.goff, P, 4);
    r.hcand = WsPart{ws_align_up(r.nflat.end(), 16), P * kHintCands, kHintCandBytes, 16};
    r.snap_bytes = r.cnt.end();
    // (the sum of the parts plus the slack of the two round-ups, the goff tail and spare)
    r.bytes = r.r2list.end() + 64 + r.gref.count * kFloat4Bytes + r.gsel.count * 4 + P * 8 + 128 +
              P * 4 + 16 + r.hcand.count * kHintCandBytes;

    auto& s = l.sortbuf;
    s.len = (size_t)sortbuf_len(iters);
    s.score = WsPart{0, P * s.len, 4, 4};
    s.list2 = s.score;
    s.list2_bounds_stride = S;
    s.list2_refine_stride = s.len;
    s.bytes = s.score.end();

    auto& h = l.hlite;
    h.hl = WsPart{0, P * 9 * (size_t)iters, 4, 4};
    h.wsum = after(h.hl, P * (((size_t)iters + 63) / 64) * 8, 4);
    h.bytes = h.wsum.end();

    auto& t = l.rtab;
    t.recip = WsPart{0, (size_t)kRecipTable, 8, 8};
    t.magic = after(t.recip, (size_t)kRecipTable, 8);
    t.bad = after(t.magic, 1, 4);
    t.bytes = (size_t)kRecipTable * 16 + 8;
    return l;
}

}  // namespace erp

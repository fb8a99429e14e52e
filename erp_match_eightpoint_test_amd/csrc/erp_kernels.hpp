// erp_kernels.hpp -- launchers of the gfx950 kernels (matcher.hip: the matcher; kernels.hip:
// the rest of the hot path).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/erp_match.h"
#include "erp_consensus_ws.hpp"

namespace erp {

constexpr int kDim = 64;          // SURF descriptor length (extended=false)
constexpr int kMaxQ = 24;         // jump polynomials x^(64(M-1)2^k): waves per pair < 2^24
constexpr int kPolyWords = 31;    // glibc TYPE_3 degree
#ifndef ERP_CAND_SLOTS
#define ERP_CAND_SLOTS 28
#endif
constexpr int kCandSlots = ERP_CAND_SLOTS;    // matcher: tiles with candidate rows kept per (query, train
                                  // chunk, lane half) (more: exact sweep of the chunk)

// the batch pipeline's gather + bearings (bearings_from_matches_kernel's work), done by
// knn2_merge_kernel as it places each match (src/spherical_surf.cpp:155-162 +
// src/eight_point.cpp:163-186): pts[p][max_nq + 1][6] (the last row the zero pad of the Gram
// batches), optional valid_key_left / right
struct BearingOut {
    const erp_point2f* kp_l;
    const erp_point2f* kp_r;
    const int32_t* width;
    const int32_t* height;
    double* pts;
    erp_point2f* key_l;
    erp_point2f* key_r;
};
struct Top2 {                     // partial k=2 result of one train chunk for one query
    float d0;                     // best squared distance
    int32_t j0;                   // its train index (lowest index among ties)
    float d1;                     // second squared distance
};

struct BatchShape {
    int n_pairs;
    int max_nq, max_nt;
    int fchunks, fchunk_len;      // train chunks of the matcher's MFMA filter
    int xchunks, xchunk_len;      // train chunks of the exact VALU sweep (multiples of 128)
    int iters;
    int max_s;                    // (int)(max_nq * sample_frac)
    int idx_stride;               // entries of one hypothesis in the debug samples output
    int sel_words;                // 31-step selection words per hypothesis (>= (M-1)/31 + 1)
    // route options (erp_ctx_set_option; -1 / 0 = automatic): the sampler's block kind and split
    // replay, the Gram kernel's row tiles per wave, the throughput sampler's launch tiers
    int sampler_lat = -1, sampler_split = -1, gram_tiles = 0, sampler_tiers = -1;
    // words between the pairs' glibc start windows (launch_sampler's w0): 0 = one window shared
    // by every pair (cfg's seed / offset), 31 = one per pair (a rand stream, rand_stream.hip)
    int w0_stride = 0;
    // the launch's alias table (launch_sampler_alias: rep[p] = the pair whose jump polynomials,
    // windows and selection words pair p uses); null = every pair produces and reads its own
    const int32_t* rep = nullptr;
};

hipError_t launch_set_i32(int32_t* p, int32_t v, hipStream_t st);  // (values via kernel args:
hipError_t launch_set_i64x4(int64_t* p, int64_t a, int64_t b, int64_t c, int64_t d,  // no host
                            hipStream_t st);                                       // lifetime)
void init_constants();            // reduction table for the jump polynomials (once per device)

// matcher: knn2_filter (train rows split to bf16, then ONE MFMA pass: per-(query, chunk) top-2
// upper bounds pu, and per (query, chunk, lane half) up to kCandSlots tiles that may hold
// candidates: the tile and its 16 bounds of the lane's rows; counts in ccount), rescore (exact
// Top2 per (query, chunk) of the stored rows under the final bound into
// part[pairs][fchunks][max_nq]), merge (ratio + compaction).  split = scratch of
// knn2_split_bytes(sh) (bf16 rows, norms, per-pair max norm); cand = knn2_cand_bytes(sh).
size_t knn2_split_bytes(const BatchShape& sh);
size_t knn2_cand_bytes(const BatchShape& sh);
// (ovf: the rescore's overflow scratch below; its counter ovf[0] is zeroed here)
hipError_t launch_knn2_filter(const float* desc_q, const float* desc_t, const int64_t* off_q,
                              const int64_t* off_t, const BatchShape& sh, void* split,
                              float2* pu, int32_t* ccount, void* cand, hipStream_t st,
                              int32_t* ovf, int32_t* flags);  // flags [n_pairs] zeroed (may be null)
// ovf = scratch of 4 + 12 * n_pairs * max_nq * fchunks bytes: overflowed (pair, query, chunk)
// for the exact sweep (counter zeroed by the launch_knn2_filter before it)
hipError_t launch_knn2_rescore(const float* desc_q, const float* desc_t, const int64_t* off_q,
                               const int64_t* off_t, const BatchShape& sh, void* split,
                               const float2* pu, const int32_t* ccount, void* cand, Top2* part,
                               int32_t* ovf, float ratio, hipStream_t st);
// exact sweep on packed FP32 VALU (no MFMA filter): per-(chunk, query) exact k=2 into
// xpart[pairs][xchunks][max_nq]
hipError_t launch_knn2_exact(const float* desc_q, const float* desc_t, const int64_t* off_q,
                             const int64_t* off_t, const BatchShape& sh, Top2* xpart,
                             hipStream_t st);
// per-chunk partials part[pairs][chunks][max_nq] -> one Top2 per query out[pairs][max_nq]
hipError_t launch_knn2_fold(const Top2* part, const int64_t* off_q, const int64_t* off_t,
                            const BatchShape& sh, int chunk_len, int chunks, Top2* out,
                            hipStream_t st);
// fold of per-chunk partials part[pairs][chunks][max_nq] (chunk c = train rows
// [c*chunk_len, (c+1)*chunk_len)), ratio test, compaction
size_t knn2_merge_scratch_bytes(const BatchShape& sh);
hipError_t launch_knn2_merge(const Top2* part, const int64_t* off_q, const int64_t* off_t,
                             const BatchShape& sh, int chunk_len, int chunks, float ratio,
                             erp_dmatch* matches, int32_t* counts, int32_t* flags,
                             int32_t* bcount, hipStream_t st,
                             const BearingOut* bo = nullptr);
hipError_t launch_bearings_direct(const erp_point2f* kl, const erp_point2f* kr, int32_t m,
                                  int32_t W, int32_t H, double* pts, hipStream_t st);
hipError_t launch_jump_prep(const int32_t* counts, const BatchShape& sh, uint32_t* polyR,
                            uint32_t* polyQ, hipStream_t st);
// Shared replays (ERP_OPT_SAMPLER_SHARE).  With one start window for every pair (w0_stride = 0)
// and with the Philox sampler, a pair's selection words depend on its match count alone, so pairs
// of one launch with equal counts share one replay: rep[p] = the smallest q <= p with
// counts[q] == counts[p], p itself for a pair the samplers skip ((int)(M sample_frac) < 1 or
// M < 2).  One block, no host sync; launches of at most kAliasMaxPairs pairs
// (hipErrorInvalidValue above: the caller then leaves BatchShape::rep null).  Put the table into
// BatchShape::rep for launch_jump_prep, launch_sampler, launch_philox_sampler and
// launch_gram_mfma; never with per-pair start windows (w0_stride != 0).
constexpr int kAliasMaxPairs = 1024;
hipError_t launch_sampler_alias(const int32_t* counts, const BatchShape& sh, double sample_frac,
                                int32_t* rep, hipStream_t st);
// ---- rand stream (rand_stream.hip): glibc rand() state that continues from call to call ----
// host: polynomials mod P(x) = x^31 - x^28 - 1 over Z/2^32 (31 coefficients) and windows
void glibc_poly_pow(uint64_t e, uint32_t out[31]);                   // x^e mod P, by squaring
void glibc_poly_apply(const uint32_t c[31], uint32_t win[31]);       // win <- c(x) . win
void glibc_window_jump(uint32_t win[31], uint64_t n);                // win <- the window n draws on
// the sequential recurrence: the window before draw `offset` of a stream seeded with `seed`
void glibc_window_seq(uint32_t seed, uint64_t offset, uint32_t out[31]);
// device state of a stream, uint32 words: window [0, 31), seed [31], draws consumed [32, 34)
// (u64), the next window [34, 65) and next draws [66, 68) between an assign and its commit
constexpr int kStreamWin = 0, kStreamSeed = 31, kStreamDraws = 32, kStreamNextWin = 34,
              kStreamNextDraws = 66, kStreamStateWords = 72;
void init_stream_constants();     // the stream kernels' reduction table (once per device)
// the current device's power table x^(k 256^j) (256 KB of device memory, built on first use):
// blocking, so call it before a capture; false when it could not be allocated
bool stream_tables_ready();
// One consuming launch: pair p's start window w0s[p][31] = the window e_p draws past the
// stream's, e_p = sum over q < p of d_q, d_q = iters (M_q - 1) for a pair the sampler runs
// ((int)(M_q sample_frac) >= 1 and M_q >= 2) and 0 otherwise (its window is not written); then
// the stream advances by the sum of every d_q (two kernels: assign, commit).
hipError_t launch_stream_assign(const int32_t* counts, int n_pairs, int iters, double sample_frac,
                                uint32_t* state, uint32_t* w0s, hipStream_t st);
// set != 0: state <- (seed, n draws consumed); else the state advances by n draws (one wave)
hipError_t launch_stream_jump(uint32_t* state, int set, uint32_t seed, uint64_t n,
                              hipStream_t st);

// part 0: lane end windows (jump-ahead); part 1: the backwards replay -> selection bitmaps
hipError_t launch_sampler(const int32_t* counts, const uint32_t* polyR, const uint32_t* polyQ,
                          const uint32_t* w0, const BatchShape& sh, double sample_frac,
                          const double* rtab, uint32_t* wins, uint32_t* selw, int32_t* flags,
                          hipStream_t st, int part);
// rtab[d] = 1/d rounded up, d < kRecipTable (the sampler's exact modulo); *bad counts entries
// whose one-sided error bound fails (never, by construction; checked once per context).  The
// table allocation (reciprocals, magic numbers, check counter): ConsensusLayout::rtab
// host: mtab[d] = m_d | (l_d - 1) << 32 (kernels.hip mod_magic_i24); false if a divisor fails
// the exact Granlund-Montgomery condition (never, by construction)
bool build_magic_table(uint64_t* mtab, int n);
// the counter-based sampler (ERP_SAMPLER_PHILOX): selection words in the replay's format,
// max_m = the batch's largest M (<= max_nq); hipErrorInvalidValue when M's bitmap exceeds LDS
hipError_t launch_philox_sampler(const int32_t* counts, const BatchShape& sh, double sample_frac,
                                 uint32_t seed, uint64_t offset, int max_m, uint32_t* selw,
                                 int32_t* flags, hipStream_t st);
hipError_t launch_recip_table(int n, double* rtab, int32_t* bad, hipStream_t st);
int debug_lip_counters(uint32_t* out64);
// Gram of every iteration's sample on int8 MFMA (exact fixed-point sums) -> gram[p][36][iters];
// limbs = scratch of gram_limbs_bytes(sh); samples (debug, may be NULL) = the sampled indices.
// evec != NULL fuses the eigen stage's inverse iteration (pairs with s >= 9) into the Gram
// kernel: evec[p][9][iters] written there, and the Gram written to HBM only for pairs with
// s < 9 and for the iterations whose inverse iteration did not settle (evec NaN); then call
// launch_eigen with fused = 1.  hyps != NULL as well: the settled lanes' estimates too (fused = 2:
// the fallback and thin eigen kernels then write their own lanes' records, no estimate_kernel)
// sh.rep != NULL: pair p reads pair rep[p]'s selection words, and flags [n_pairs] (required
// then) gets the representative's sampler consistency bit for each aliased pair
size_t gram_limbs_bytes(const BatchShape& sh);
hipError_t launch_gram_mfma(const int32_t* counts, const double* pts, const uint32_t* selw,
                            const BatchShape& sh, double sample_frac, int8_t* limbs,
                            double* gram, int32_t* samples, double* evec,
                            erp_hypothesis* hyps, double valid_abs, hipStream_t st,
                            int32_t* flags = nullptr);

// selected singular vector per iteration from the Grams gram[p][36][iters] -> evec[p][9][iters],
// then the estimate (rank-2 fix, decomposition, Euler angles, validity) -> hyps
hipError_t launch_eigen(const int32_t* counts, const double* gram, const BatchShape& sh,
                        double sample_frac, double valid_abs, double* evec, erp_hypothesis* hyps,
                        hipStream_t st, int fused = 0, bool want_e = true,
                        float* hl = nullptr, int32_t* wsum = nullptr);
// (hl != NULL, round 5: the estimates go to the lite layout -- hl[p][9][iters] f32 R1, R2, T,
// an invalid rotation's x NaN, plus per-64-iteration-wave counts / bounding boxes wsum -- the
// two parts of ConsensusLayout::hlite, for launch_valid_place instead of records)
// (want_e = false: estimate_kernel leaves the records' E unwritten -- the batch pipeline when the
// caller did not ask for the hypothesis records; nothing downstream reads E)
// the opt-in inlier count (cfg.inlier_thr > 0): every iteration's matches with
// |l^T E' r| < thr into hyps[p][iters].inliers (the records' E must be written); scratch of
// inlier_scratch_bytes(sh)
size_t inlier_scratch_bytes(const BatchShape& sh);
hipError_t launch_inliers(const int32_t* counts, const double* pts, const BatchShape& sh,
                          double sample_frac, float thr, void* scratch, erp_hypothesis* hyps,
                          hipStream_t st);
// R_vec_arr / T_vec_arr in push order + K + bounding-box scale; vchunk = scratch of
// valid_chunk_bytes(sh) (per 1024-iteration chunk: count and bounding box)
size_t valid_chunk_bytes(const BatchShape& sh);
hipError_t launch_valid_compact(const int32_t* counts, const erp_hypothesis* hyps,
                                const BatchShape& sh, double sample_frac, int32_t* vchunk,
                                float* rv, float* tv, int32_t* kcount, float* rv_aos,
                                float* dscale, hipStream_t st);
// The winner stage (winner.hip; include/erp_match.h "winner records"), after the consensus: per
// pair the iteration that pushed row min_idx -- from the records' flags (hyps != NULL) or from
// the lite estimates' NaN marks and per-wave counts (hl, wsum: ConsensusLayout::hlite) -- its
// Gram re-summed from the selection words selw (pair rep[p]'s when rep != NULL) over pts, the
// pipeline's solve, and the self-check against results[p].  Reads only; one launch.
struct WinnerArgs {
    const erp_pair_result* results;   // [P]
    const erp_hypothesis* hyps;       // [P][iters], or null: the lite route
    const float* hl;                  // [P][9][iters] (lite)
    const int32_t* wsum;              // [P][nwaves][8] (lite)
    const int32_t* counts;            // [P] M
    const double* pts;                // [P][max_nq + 1][6]
    const uint32_t* selw;             // [P][nwaves][nbw][64]
    const int32_t* rep;               // [P] or null
    int iters, nwaves, nbw, max_nq;
    double sample_frac, valid_abs;
    erp_winner* out;                  // [P]
};
hipError_t launch_winner(const WinnerArgs& a, int n_pairs, hipStream_t st);
// The support stage (support.hip; include/erp_match.h "support-scored winner"), after the
// consensus: every iteration's inlier count under thr, the best-supported scored iteration per
// pair and its records.  It reads what the run left (the records, or evec / gram / hl of the lite
// route; counts, pts) and writes only its own scratch and the caller's outputs.  Four launches.
struct SupportScratch {               // support_scratch(sh): the padded extents and the parts
    int ipad, mpad;                   // iterations / matches rounded up to the kernels' tiles
    size_t ec64_bytes, eimg_bytes, xflag_bytes, uimg_bytes, counts_bytes;
};
struct SupportArgs {
    const erp_pair_result* results;   // [P] the run's records
    const erp_hypothesis* hyps;       // [P][iters], or null: the lite route
    const double* evec;               // [P][9][iters] (lite)
    const double* gram;               // [P][36][iters] (lite)
    const float* hl;                  // [P][9][iters] (lite)
    const int32_t* mcount;            // [P] M
    const double* pts;                // [P][max_nq + 1][6]
    int iters, ipad, max_nq, mpad;
    int mfma;                         // the count's fast evaluation: 1 bf16 MFMA, 0 f32 VALU
    double sample_frac, valid_abs, thr;
    float thr_lo, thr_hi;             // support_band(thr, mfma)
    double* ec64;                     // scratch [P][iters][9]: E' (the exact path)
    void* eimg;                       // scratch [P][ipad] x 64 B: E' as the count's operand
    int32_t* xflag;                   // scratch [P][ipad]: iterations counted in fp64 only (MFMA)
    void* uimg;                       // scratch [P][mpad] x 64 B: u = l (x) r as the operand
    int32_t* counts;                  // [P][iters] (the caller's, or scratch)
    erp_support* support;             // [P]
    erp_winner* winners;              // [P] or null
    erp_pair_result* out_results;     // [P] or null
};
SupportScratch support_scratch(const BatchShape& sh);
// the f32 constants of the count's band: |x| < lo is an inlier, |x| >= hi is not
void support_band(double thr, bool mfma, float* lo, float* hi);
hipError_t launch_support(const SupportArgs& a, int n_pairs, hipStream_t st);
hipError_t launch_gram_all(const double* pts, int32_t m, double* gram, hipStream_t st);
hipError_t launch_consensus_input(const float* rvec, const float* tvec, int K, int stride, float* rv,
                                  float* tv, int32_t* kcount, float* dscale, int32_t* flags,
                                  hipStream_t st);

// The consensus stage's device pointers: the context's scratch buffers by their base (what is
// where inside them is erp_consensus_ws.hpp's business, turned into typed pointers by
// kernels.hip consensus_views) and the call's inputs / outputs.
struct ConsensusBufs {
    const int32_t* counts;        // [P] M (null when the valid list was given directly)
    const int32_t* flags;         // [P] internal error flags
    int32_t* kcount;              // [P] K
    float* rv;                    // [P][3][2 iters] valid R (SoA)
    float* tv;                    // [P][2 iters][3] their T (the context's or the caller's)
    float* rv_aos;                // optional output R_vec_arr (may be null)
    float* dscale;                // [P] bounding-box scale
    double* tmean;                // [P][2 iters] (the context's or the caller's)
    double* lb;                   // lb / ub / bsel: the context's, or the caller's own for the
    double* ub;                   // row-sharded entry points
    int32_t* bsel;
    void *zsel, *surv, *nsurv, *edges, *lipref, *sortbuf, *hlite;  // ConsensusLayout's buffers
    erp_pair_result* results;
};
struct ConsensusParams {
    double sample_frac, trim_lo, trim_hi;
    int shard, nshards;           // the row shard of the bounds pass (0, 1: every row)
    bool prune;                   // false = the small-batch route: every row binned, no lists
    int lip2, lipg, flat_pct, hint;  // the pruning route (capi.hip pruning_opts)
    bool edges_ready;             // launch_valid_place wrote the first-pass edges already
};
hipError_t launch_valid_place(const ConsensusBufs& b, const BatchShape& sh,
                              const ConsensusParams& cp, hipStream_t st);
// per-row [LB, UB] of the trimmed mean and the bins holding ranks lo / hi-1 (bsel[row][2])
hipError_t launch_consensus_bounds(const ConsensusBufs& b, const BatchShape& sh,
                                   const ConsensusParams& cp, hipStream_t st);
hipError_t launch_consensus_zoom(const ConsensusBufs& b, const BatchShape& sh,
                                 const ConsensusParams& cp, int level, hipStream_t st);
// survivors = rows with LB <= min UB (again = 1: only pairs the refine pass touched)
hipError_t launch_consensus_select(const ConsensusBufs& b, const BatchShape& sh,
                                   const ConsensusParams& cp, int again, hipStream_t st);
// tighter [LB, UB] for the current survivors (exact inner sums + sub-bins of the boundary bins)
hipError_t launch_consensus_refine(const ConsensusBufs& b, const BatchShape& sh,
                                   const ConsensusParams& cp, hipStream_t st);
hipError_t launch_consensus_rows(const ConsensusBufs& b, const BatchShape& sh,
                                 const ConsensusParams& cp, hipStream_t st);
hipError_t launch_consensus_final(const ConsensusBufs& b, const BatchShape& sh,
                                  const ConsensusParams& cp, hipStream_t st);
// after row-sharded bounds (not combined over the shards): binned rows = -1 for every pair
hipError_t consensus_mark_unbinned(const ConsensusBufs& b, const BatchShape& sh, hipStream_t st);
// debug snapshot right after the bounds pass: lb, ub [P][2 iters] f64, the first-stage list
// counts [P] i32 (-1 without pruning), then the first-stage references (float4 [P][cap]), their
// U [P] f64 and counts [P] i32; dst = device memory of consensus_snapshot_bytes(sh)
size_t consensus_snapshot_bytes(const BatchShape& sh);
hipError_t consensus_snapshot(const ConsensusBufs& b, const BatchShape& sh,
                              const ConsensusParams& cp, void* dst, hipStream_t st);

}  // namespace erp

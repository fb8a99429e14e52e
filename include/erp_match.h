/*
 * erp_match.h -- C ABI of the MI355X-native ERP matcher + spherical eight-point estimator.
 *
 * This is the drop-in boundary for the reference's hot path (Kitsunetic/ERP_match_eightpoint_test):
 *
 *   erp_match_two_image / erp_match_knn2_ratio
 *       replaces  std::vector<cv::DMatch> feature_matcher::match_two_image(
 *                     const cv::Mat& descriptor1, const cv::Mat& descriptor2)
 *                 /root/reference/src/feature_matcher.hpp:36, body src/feature_matcher.cpp:42-59
 *                 (FLANN knnMatch k=2 + ratio 0.3f; here: EXACT k=2 in flann::L2 order).
 *   erp_eight_point_find
 *       replaces  void eight_point::find(int im_width, int im_height,
 *                     std::vector<cv::KeyPoint>& key_left, std::vector<cv::KeyPoint>& key_right,
 *                     cv::Vec3f& R_vec_out, cv::Vec3f& T_vec_out, int match_size)
 *                 /root/reference/src/eight_point.hpp:11-14, body src/eight_point.cpp:152-192
 *                 (initial_guess :87-150 and the random_array sampler eight_point.hpp:30-59 run
 *                  inside; the iteration count, sample fraction, trim window and validity bound
 *                  are the hard-coded constants of :99,:102,:143,:76 exposed in erp_ransac_cfg).
 *   erp_eight_point_estimation
 *       replaces  void eight_point::eight_point_estimation(int, int, std::vector<cv::Point3d>&,
 *                     std::vector<cv::Point3d>&, cv::Vec3f& R1, cv::Vec3f& R2, cv::Vec3f& T,
 *                     bool& R1_valid, bool& R2_valid, int match_size)
 *                 /root/reference/src/eight_point.hpp:15-19, body src/eight_point.cpp:16-85
 *   erp_pair_batch_run
 *       the fused hot path for many ERP pairs at once: spherical_surf::do_all's
 *       match -> gather (src/spherical_surf.cpp:153-162, 177) -> eight_point::find
 *       (src/automatic.cpp:117-126 calls exactly this sequence per pair).
 *
 * Conventions: plain C types only; `void* stream` is a hipStream_t (NULL = default stream);
 * device-pointer entry points are asynchronous on that stream, host-pointer ones synchronous.
 * A context (erp_ctx) owns grow-only scratch that every call on it reuses, so calls on one
 * context are serialised on the device: a call enqueued on a different stream than the previous
 * call on the same context first waits (hipStreamWaitEvent) for that call's work to finish.
 * Independent work that should overlap needs one context per stream.  Calls are thread-safe
 * (one lock per context; host-pointer calls hold it across upload, run and download).
 * No C++ exception crosses this boundary; every call returns an erp_status.  The reference's
 * undefined behaviour cases are given explicit statuses (see erp_status).
 */
#ifndef ERP_MATCH_H
#define ERP_MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ERP_MATCH_ABI_VERSION 2  /* 2: erp_ctx_set_option replaced the environment knobs (r06) */

typedef enum erp_status {
    ERP_OK = 0,
    ERP_INVALID_ARG = 1,
    ERP_TOO_FEW_POINTS = 2,       /* train set < 2 (knn_matches[i][1] UB, feature_matcher.cpp:52),
                                     or (int)(M*sample_frac) < 1 (A_mat with 0 rows, :18) */
    ERP_NO_VALID_HYPOTHESIS = 3,  /* K == 0: R_vec_arr[min_idx] on an empty vector (:148) */
    ERP_HIP_ERROR = 4,
    ERP_NO_DEVICE = 5,
    ERP_OUT_OF_MEMORY = 6,
    ERP_INTERNAL = 7
} erp_status;

/* cv::DMatch layout */
typedef struct erp_dmatch {
    int32_t queryIdx;
    int32_t trainIdx;
    int32_t imgIdx;
    float distance;
} erp_dmatch;

/* cv::KeyPoint::pt (the only KeyPoint field the hot path reads) */
typedef struct erp_point2f {
    float x;
    float y;
} erp_point2f;

typedef enum erp_sampler {
    ERP_SAMPLER_GLIBC = 0, /* replay of glibc rand() + libstdc++ random_shuffle (the reference) */
    ERP_SAMPLER_PHILOX = 1 /* counter-based, no reference counterpart:
                              iteration h's subset by Floyd's algorithm on Philox4x32-10 draws,
                              h = offset + iteration (offset counts iterations, not rand() calls);
                              the exact definition: oracle/erp_oracle.c erpo_philox_sample.
                              A pair with more than 20480 matches (the per-lane LDS bitmap)
                              gets ERP_INVALID_ARG. */
} erp_sampler;

/* initial_guess parameters; erp_ransac_cfg_default() gives the reference constants. */
typedef struct erp_ransac_cfg {
    int32_t iters;       /* 80   src/eight_point.cpp:99 */
    int32_t sampler;     /* ERP_SAMPLER_GLIBC (the reference) or ERP_SAMPLER_PHILOX */
    double sample_frac;  /* 0.25 :102 */
    double trim_lo;      /* 0.2  :143 */
    double trim_hi;      /* 0.8  :143 */
    double valid_abs;    /* 1.57 :76,81.  A rotation is valid when every |Euler angle| < valid_abs,
                            so valid_abs <= 0 or NaN makes none valid: every pair that reaches
                            the consensus gets K = 0 and ERP_NO_VALID_HYPOTHESIS (the hypothesis
                            records are still written, every flag 0) -- accepted, not an
                            ERP_INVALID_ARG.  valid_abs > pi makes every finite rotation valid:
                            K = 2 iters */
    uint32_t seed;       /* 1: the reference never calls srand() */
    float inlier_thr;    /* 0 (default) = off: nothing below changes.  > 0: every iteration also
                            counts its inliers, the correspondences with |l^T E' r| < inlier_thr
                            (l, r the unit bearings of a match, E' = E_mat_correct of that
                            iteration, src/eight_point.cpp:46-50: the rank-2 correction of the
                            unit-norm solved e), into erp_hypothesis.inliers (the winner's count:
                            the record of the iteration that pushed row min_idx).  No reference
                            counterpart (its loop, :99-127, keeps no score): the opt-in
                            "inlier count" of SURVEY.md F2.  Exact definition (fp64, fixed
                            order): u_k = l_i * r_j (k = 3i + j), res = E'_0 u_0, then
                            res = fma(E'_k, u_k, res) for k = 1..8; inlier iff |res| < thr
                            (oracle/erp_oracle.c erpo_inlier_count). */
    uint64_t offset;     /* rand() calls consumed before initial_guess (e.g. by FLANN) */
} erp_ransac_cfg;

/* one initial_guess iteration (R1, R2, T as Vec3f; E = the solved 9-vector, sign arbitrary) */
typedef struct erp_hypothesis {
    float R1[3];
    float R2[3];
    float T[3];
    int32_t R1_valid;
    int32_t R2_valid;
    int32_t inliers;     /* matches with |l^T E' r| < cfg.inlier_thr (erp_ransac_cfg); 0 when off */
    double E[9];
} erp_hypothesis;

/* per-pair result of find / the batch pipeline */
typedef struct erp_pair_result {
    float R[3];          /* R_vec_out (XYZ Euler, rad) */
    float T[3];          /* T_vec_out (unit) */
    int32_t status;      /* erp_status of this pair */
    int32_t M;           /* matches after the ratio test (match_size) */
    int32_t K;           /* valid rotation hypotheses */
    int32_t min_idx;     /* consensus winner in R_vec_arr order */
    int32_t sample_n;    /* (int)(M * sample_frac) */
    int32_t near_ties;   /* rows re-scored exactly by the near-tie resolver */
    int32_t survivors;   /* rows whose trimmed-mean bounds did not exclude them (a diagnostic:
                            it depends on which pruning references ran, so a row-sharded
                            consensus -- erp_consensus_hyps_shard/finish_dev -- may report a
                            different count than the unsharded one; 1 <= survivors <= K, and
                            <= binned_rows when that is reported) */
    int32_t binned_rows; /* rows whose K-column distance histogram was built (K, or the
                            reference rows + the rows Lipschitz pre-pruning kept; K on the
                            row-sharded path, whose shards do not combine it) */
    double min_dist;     /* trimmed-mean distance of the winner */
} erp_pair_result;

/* device pointers describing a batch of ERP pairs (rows concatenated pair after pair) */
typedef struct erp_pair_batch {
    int32_t n_pairs;
    int32_t dim;                /* descriptor length (64 for SURF; the fast path needs 64) */
    int32_t max_nq;             /* host-known upper bound of rows per pair (queries / left) */
    int32_t max_nt;             /* ... (train / right) */
    const float* desc_l;        /* [sum nq][dim] queries  (descriptor1) */
    const float* desc_r;        /* [sum nt][dim] train    (descriptor2) */
    const erp_point2f* kp_l;    /* [sum nq] keypoints of desc_l rows */
    const erp_point2f* kp_r;    /* [sum nt] */
    const int64_t* off_l;       /* [n_pairs+1] row offsets into desc_l / kp_l */
    const int64_t* off_r;       /* [n_pairs+1] */
    const int32_t* width;       /* [n_pairs] ERP width  (im_width) */
    const int32_t* height;      /* [n_pairs] ERP height (im_height) */
} erp_pair_batch;

/* optional device outputs of the batch pipeline (NULL = not needed) */
typedef struct erp_batch_outputs {
    erp_pair_result* results;   /* [n_pairs] (required) */
    erp_dmatch* matches;        /* [n_pairs][max_nq], queryIdx/trainIdx local to the pair */
    erp_point2f* key_left;      /* [n_pairs][max_nq] gathered matched keypoints (valid_key_left) */
    erp_point2f* key_right;     /* [n_pairs][max_nq] */
    erp_hypothesis* hyps;       /* [n_pairs][iters] */
    int32_t* samples;           /* [n_pairs][iters][max sample_n] sampled match indices (as a set,
                                   order unspecified) */
    float* rvec;                /* [n_pairs][2*iters][3] R_vec_arr */
    float* tvec;                /* [n_pairs][2*iters][3] T_vec_arr */
    double* dist;               /* [n_pairs][2*iters] trimmed means of the rows that survive the
                                   bounds test (exact order statistics, fp64 sum; near ties are
                                   re-scored with the reference's sorted sequential sum); +inf for
                                   rows proven not to be the minimum */
} erp_batch_outputs;

typedef struct erp_ctx erp_ctx;

/* ---- context ---- */
erp_status erp_ctx_create(int32_t device, erp_ctx** out);
erp_status erp_ctx_destroy(erp_ctx* ctx);
const char* erp_status_string(erp_status s);
void erp_ransac_cfg_default(erp_ransac_cfg* cfg);
int32_t erp_abi_version(void);
/* Pre-size device scratch so later calls allocate nothing (graph-capture friendly). */
erp_status erp_ctx_reserve(erp_ctx* ctx, int32_t n_pairs, int32_t max_nq, int32_t max_nt,
                           int32_t iters);

/* ---- rand stream: the glibc rand() stream continued from call to call ----
   The reference draws from glibc's process-global rand(): every eight_point::find of a process
   goes on where the previous one stopped (one_image_test/main.cpp:135-137,
   two_real_image_test/main.cpp:283-286; epipolar_tool.cpp:15 shuffles on the same stream).
   Without a stream every call starts at (cfg->seed, cfg->offset), as it always did.  A rand
   stream holds (seed, draws consumed, the 31-word glibc window); attached to a context
   (erp_ctx_set_rand_stream) it replaces cfg->seed / cfg->offset in the CONSUMING calls:
       erp_eight_point_find, erp_eight_point_find_dev, erp_initial_guess, erp_pair_batch_run,
       erp_image_pairs_run, their *_winner(s) forms (and erp_epipolar_draw_dev, which shuffles
       on it);
   these ignore cfg->seed and cfg->offset, draw from the stream and advance it.  NOT consuming:
   erp_eight_point_hypotheses_dev and the erp_consensus_* calls, which reproduce blocks of a
   larger find at an explicit offset and stay on cfg->offset.  ERP_SAMPLER_PHILOX on a context
   with a stream gives ERP_INVALID_ARG.
   Consumption rule: a pair consumes iters * (M - 1) draws when the sampler runs it, that is
   when (int)(M * sample_frac) >= 1 and M >= 2 -- whatever its final status, K == 0 included --
   and 0 draws otherwise (the reference is undefined there: src/eight_point.cpp:101-116 with
   sample_n == 0).  The pairs of a batch consume in pair order: pair p starts
   iters * sum_{q<p, q consuming} (M_q - 1) draws past the stream's position at the call.  The
   M_q stay on the device: a kernel hands every pair its start window and advances the state,
   with no host round trip.  The counter wraps mod 2^64; the window stays the true one.
   Order and threads: a stream may be attached to several contexts.  Calls serialise on the
   stream (its own lock, and on the device an event recorded right after the kernel that
   advances the state, which the next consumer on any HIP stream waits for): results follow the
   order in which the calls take the stream, and overlapped calls on different contexts wait
   for that kernel only, not for each other's pipelines.  Under erp_ctx_set_graphs the state
   and the per-pair windows sit at fixed device addresses, so a replayed graph continues the
   stream (the whole graph launch is then the stream's turn).  A stream must outlive its
   attachment: detach (erp_ctx_set_rand_stream(ctx, NULL)) before erp_rand_stream_destroy.
   The state lives on the host until the first GPU call uses the stream, from then on in that
   device's memory (a stream serves one device). */
typedef struct erp_rand_stream erp_rand_stream;
/* host only until the first device use (works without a GPU): the stream seeded with `seed`
   (0 = 1, as srand) after `offset` draws; positioning costs O(log offset) */
erp_status erp_rand_stream_create(uint32_t seed, uint64_t offset, erp_rand_stream** out);
erp_status erp_rand_stream_destroy(erp_rand_stream* s);
/* (seed, draws consumed) after the stream's last device update (waits for it) */
erp_status erp_rand_stream_get(erp_rand_stream* s, uint32_t* seed, uint64_t* draws);
erp_status erp_rand_stream_set(erp_rand_stream* s, uint32_t seed, uint64_t offset);
/* skip n draws: how a host accounts for rand() calls made elsewhere (FLANN) between calls */
erp_status erp_rand_stream_advance(erp_rand_stream* s, uint64_t n);
/* the process-wide stream of a device, created at (1, 0) on first request: the reference's
   process-global state.  Never destroyed by the caller. */
erp_status erp_rand_stream_process(int32_t device, erp_rand_stream** out);
/* s = NULL detaches */
erp_status erp_ctx_set_rand_stream(erp_ctx* ctx, erp_rand_stream* s);
erp_status erp_ctx_get_rand_stream(erp_ctx* ctx, erp_rand_stream** out);
/* erp_random_shuffle_prefix drawing from the stream: consumes m - 1 draws (0 for m < 2) */
erp_status erp_rand_stream_shuffle_prefix(erp_rand_stream* s, int32_t m, int32_t n,
                                          int32_t* h_idx);

/* ---- stage timing (the reference's START_TIME/STOP_TIME, src/debug_print.h:9-13, applied to
   the hot path): HIP events recorded around every kernel on the pipeline's stream. ---- */
typedef enum erp_stage {
    ERP_STAGE_KNN2_FILTER = 0,  /* bf16 split + the one MFMA pass: bounds + provisional candidates */
    ERP_STAGE_KNN2_MERGE = 1,   /* chunk fold + ratio test + compaction */
    ERP_STAGE_BEARINGS = 2,     /* gather + pixel -> bearing */
    ERP_STAGE_JUMP_PREP = 3,    /* glibc jump-ahead polynomials (and, on a rand stream, the
                                   kernels that hand out the pairs' start windows) */
    ERP_STAGE_SAMPLER = 4,      /* random_array replay (glibc, backwards, bitmap) */
    ERP_STAGE_EIGEN = 5,        /* 9x9 Jacobi, rank-2 fix, decomposeEssentialMat, Euler */
    ERP_STAGE_VALID_COMPACT = 6,
    ERP_STAGE_CONSENSUS_ROWS = 7,   /* exact order statistics of the surviving rows */
    ERP_STAGE_CONSENSUS_FINAL = 8,
    ERP_STAGE_CONSENSUS_BOUNDS = 9, /* per-row trimmed-mean bounds (one pass over K^2) */
    ERP_STAGE_CONSENSUS_SELECT = 10,
    ERP_STAGE_WINDOWS = 11,         /* per-iteration glibc end windows (jump-ahead) */
    ERP_STAGE_GRAM = 12,            /* A^T A of every sample (fp64) */
    ERP_STAGE_KNN2_CANDIDATES = 13, /* unused since r02 (the two MFMA passes were fused) */
    ERP_STAGE_KNN2_RESCORE = 14,    /* exact flann::L2 distances of the candidates */
    ERP_STAGE_CONSENSUS_REFINE = 15, /* tighter bounds for the survivors (sub-bins) */
    ERP_STAGE_KNN2_EXACT = 16,      /* exact sweep on packed FP32 VALU (ERP_MATCHER_VALU_EXACT) */
    ERP_STAGE_SAMPLER_GRAM = 17,    /* unused since r06 (the fused sampler + Gram kernel, slower, was removed) */
    ERP_STAGE_INLIERS = 18,         /* opt-in per-iteration inlier count (cfg.inlier_thr > 0) */
    ERP_STAGE_COUNT = 19
} erp_stage;
erp_status erp_ctx_set_profiling(erp_ctx* ctx, int32_t enable);
const char* erp_stage_name(int32_t stage);
/* Waits for the recorded events, writes per-stage total milliseconds and launch counts
   (arrays of ERP_STAGE_COUNT), then clears the record. */
erp_status erp_ctx_stage_times(erp_ctx* ctx, double* total_ms, int64_t* launches);

/* ---- matcher (feature_matcher::match_two_image) ---- */
/* How the exact k=2 is computed (both give the same bit-exact matches):
   MFMA_FILTER: bf16 MFMA upper/lower bounds -> candidates -> exact flann::L2 rescoring (default);
   VALU_EXACT:  every distance exactly, LDS-tiled packed FP32 sweep (configs[3]'s scalar path). */
typedef enum erp_matcher_method {
    ERP_MATCHER_MFMA_FILTER = 0,
    ERP_MATCHER_VALU_EXACT = 1
} erp_matcher_method;
erp_status erp_ctx_set_matcher(erp_ctx* ctx, int32_t method);
/* enable != 0: erp_pair_batch_run captures its launch sequence (every kernel and memset of the
   pipeline, ~60 nodes) into a HIP graph the first time it sees a (batch, cfg, outputs, ratio,
   scratch) combination and replays that graph on later calls with the same one -- one launch
   instead of ~60, for the latency of small batches (configs[1]'s single pair).  Pointers are
   baked into the graph: a call with other buffers, or one that grows the context's scratch,
   captures anew (up to 8 graphs per context, least recently used dropped).  Not used while
   stage timing is on or on the NULL stream.  Default off. */
erp_status erp_ctx_set_graphs(erp_ctx* ctx, int32_t enable);
/* Route options of a context (no reference counterpart).  Each selects between code paths whose
   results are identical -- by construction, and checked by the GPU tests that set it -- and
   whose default is the measured fastest; none changes what is computed.  The library reads no
   environment variable: these setters are the only way to steer a route.  Options are part of
   a captured HIP graph's key (erp_ctx_set_graphs).  -1 = automatic where noted.
   ERP_OPT_SMALL_BATCH    consensus route: -1 auto (n_pairs (2 iters)^2 <= 2e9); n >= 0: batches
                          of <= n pairs bin every row in one pass (0 = never)
   ERP_OPT_SAMPLER_LAT    glibc replay blocks: -1 auto (latency blocks for launches of <= 1024
                          waves); 0 throughput blocks, 1 latency step by step, 2 latency with
                          the block's positions first
   ERP_OPT_SAMPLER_SPLIT  split replay: -1 auto (<= 256 workgroups); 0 off; 1 on (where its
                          bitmaps fit the LDS)
   ERP_OPT_SAMPLER_TIERS  throughput replay launches, each sizing its LDS bitmap for the pairs
                          whose sample count falls in its range: -1 auto; 0 / 1 one launch sized
                          for the batch's bound; n = 2 .. 4 at most n launches
   ERP_OPT_SAMPLER_SHARE  pairs of one launch with equal match counts share one replay (jump
                          polynomials, windows, selection words; glibc without a rand stream,
                          and Philox): -1 auto = 1 on, 0 every pair replays its own.  Never on a
                          rand stream (each pair has its own start window), for one pair, or
                          above 1024 pairs per launch.  The saving is the share of pairs that
                          repeat a count within the launch; none when all counts differ
   ERP_OPT_GRAM_TILES     32-iteration row tiles per Gram MFMA wave: 0 auto (2 once the launch
                          has >= 512 wide blocks), 1, 2
   ERP_OPT_ZOOM_LEVELS    the survivors' zoom levels 0 (default) .. 2
   ERP_OPT_SMALL_ZOOM     1: the small-batch route keeps the zoom levels (default 0)
   ERP_OPT_LIP2           second pre-pruning stage 1 / 0
   ERP_OPT_LIPG           convexity-augmented pre-pruning: bit 0 first stage (1), bit 1 second
                          stage too (3), 0 off
   ERP_OPT_REFINE_HINT    hinted refine windows 1 / 0
   ERP_OPT_FLAT_REFS      flat-pair route above this % of rows listed (25); 0 off
                          (these four: -1, the default, = automatic: the values in brackets / 1
                          for launches of >= 8 pairs, 0 below -- a few pairs with a large K, as
                          configs[4]'s one 100k-iteration find, run faster without them)
   ERP_OPT_BOUND_RATIO    the matcher's ratio test decided from the bf16 bounds where they
                          suffice 1 (default) / 0
   ERP_OPT_VERTICAL_SHARED  the vertical stage of the batched rectification
                          (erp_vertical_rotate_batch_dev, erp_rectify_batch_dev): 1 (default)
                          one shared-map launch over every image, 0 ROT90 jobs of the per-image
                          remap kernel, 8 per launch
   ERP_OPT_SUPPORT_COUNT  the support stage's per-iteration count (erp_pair_batch_run_support): -1
                          auto = 1 the bf16 MFMA product with an exact fp64 recheck of its band,
                          0 the f32 VALU chain with its (narrower) band; the counts are exact
                          either way
   ERP_OPT_STEREO_CHUNK_MB  erp_stereo_rows_dev: the MiB of S volume a chunk of pairs may take
                          in the scratch (0..1048576, default 1024; a chunk is never smaller
                          than one pair, so 0 runs the pairs one by one)
   ERP_OPT_DEBUG_STAGES   debug: bit mask of the stage groups erp_pair_batch_run enqueues (1
                          matcher + gather, 2 jump polynomials + windows, 4 sampler, 8 Gram, 32
                          eigen + estimate, 16 consensus); -1 (default) all.  A skipped group
                          leaves the previous call's scratch in place.
   ERP_OPT_DEBUG_SNAP     debug: 1 keeps a device copy of lb, ub ([P][2 iters] f64 each), the
                          first-stage list counts ([P] i32) and the first-stage Lipschitz
                          references right after the bounds pass, for erp_debug_snapshot */
typedef enum erp_ctx_option {
    ERP_OPT_SMALL_BATCH = 0,
    ERP_OPT_SAMPLER_LAT = 1,
    ERP_OPT_SAMPLER_SPLIT = 2,
    ERP_OPT_GRAM_TILES = 3,
    ERP_OPT_ZOOM_LEVELS = 4,
    ERP_OPT_SMALL_ZOOM = 5,
    ERP_OPT_LIP2 = 6,
    ERP_OPT_LIPG = 7,
    ERP_OPT_REFINE_HINT = 8,
    ERP_OPT_FLAT_REFS = 9,
    ERP_OPT_BOUND_RATIO = 10,
    ERP_OPT_DEBUG_STAGES = 11,
    ERP_OPT_DEBUG_SNAP = 12,
    ERP_OPT_SAMPLER_TIERS = 13,
    ERP_OPT_VERTICAL_SHARED = 14,
    ERP_OPT_SAMPLER_SHARE = 15,
    ERP_OPT_SUPPORT_COUNT = 16,
    ERP_OPT_STEREO_CHUNK_MB = 17,
    ERP_OPT_COUNT = 18
} erp_ctx_option;
/* ERP_INVALID_ARG for an unknown option or a value outside its range */
erp_status erp_ctx_set_option(erp_ctx* ctx, int32_t option, int32_t value);
erp_status erp_ctx_get_option(erp_ctx* ctx, int32_t option, int32_t* value);
/* debugging hooks (no reference counterpart):
   erp_debug_set_alloc_pad(N): device buffers allocated from then on get N canary bytes (0xA5)
   past their end (process-wide; 0 = off, the default); erp_debug_check_pads() returns how
   many canaries a kernel overwrote (reported on stderr).
   erp_debug_snapshot (ERP_OPT_DEBUG_SNAP) copies the snapshot to host (returns its size; host
   NULL: size only). */
void erp_debug_set_alloc_pad(size_t bytes);
int erp_debug_check_pads(void);
long long erp_debug_snapshot(erp_ctx* ctx, void* host, size_t bytes);
/* debug counters of a library built with -DERP_LIP_VERIFY=1 (the Lipschitz pruning pass
   re-checks its LDS operands against their global sources): copies 64 words into out64 and
   resets them; returns 0, -1 for a library built without the check, -2 when the copy failed. */
int erp_debug_lip_counters(uint32_t* out64);

/* device pointers; writes up to nq matches in ascending queryIdx order and *d_count. */
erp_status erp_match_knn2_ratio(erp_ctx* ctx, const float* d_query, int32_t nq,
                                const float* d_train, int32_t nt, int32_t dim, float ratio,
                                erp_dmatch* d_out, int32_t* d_count, void* stream);
/* host pointers, synchronous: the drop-in for match_two_image (ratio 0.3f). */
erp_status erp_match_two_image(erp_ctx* ctx, const float* h_desc1, int32_t n1,
                               const float* h_desc2, int32_t n2, int32_t dim,
                               erp_dmatch* h_out, int32_t* h_count);

/* ---- estimator (eight_point::find / eight_point_estimation) ----
   Input domain (tests/test_gpu_estimator_domain.py pins every rule):
   Keypoints may lie anywhere, on the image or outside it (the poles, negative or far-outside
   pixels): pixel -> bearing (src/eight_point.cpp:163-186) is periodic and gives unit bearings.
   NON-FINITE KEYPOINTS.  A pair with a NaN or Inf coordinate in a MATCHED keypoint (any of its M
   rows, sampled or not) gets the per-pair status ERP_INVALID_ARG with R = T = 0, min_idx = -1 --
   in erp_eight_point_find / _find_dev and their winner, polished and posed forms, and per pair
   in erp_pair_batch_run (the other pairs of the batch are computed as if it were not there,
   byte for byte); the winner, polish and pose records of the pair carry the status and zeros.
   A deliberate difference from the reference, which turns the pixel into NaN bearings, gets a NaN
   E from every iteration that sampled the row, finds both rotations invalid and so silently
   answers from the remaining iterations: here the status is loud, never ERP_OK with some K.
   The Gram pass sets the flag where it quantises the bearings' products; the same test refuses
   any product outside its fixed point (below), so nothing is converted or wrapped unseen.
   NON-FINITE BEARINGS.  erp_initial_guess and erp_eight_point_estimation return ERP_INVALID_ARG
   from a host check when a bearing component is NaN or Inf (no GPU work, no rand() drawn).
   BEARING SCALE.  The estimate is invariant under a scale of either side (the reference's SVD of
   A is; the oracle exactly so).  find's bearings are unit vectors.  erp_eight_point_estimation
   computes its Gram in fp64 and takes the caller's bearings as they are.  erp_initial_guess
   computes the Grams in fixed point: the products (l_a l_b)(r_c r_d) 2^44, rounded, in six
   balanced base-256 digits, which hold |product| < 7.97.  So it brings each side into the window
   first, on the host, by an exact power of two: with c = the largest |component| of a side over
   all m rows, the side is multiplied by 2^-e, e = 0 when 0.5 <= c <= 1.5 -- unit bearings
   (0.577 <= c <= 1) reach the device byte for byte -- and otherwise the e with
   0.5 <= c 2^-e < 1 (c = 0: e = 0).  Every product is then below 1.5^4 = 5.07; the Gram is
   scaled by a power of two, which leaves its eigenvectors, R and T alone: bearings times 2,
   1e-4, 1e3 or 2^40, and sides scaled differently, give the result of the unit bearings.  The
   scale is one factor per side, not per row: rows much shorter than the longest lose digits
   (a product below 2^-45 rounds to 0), so a row 1e-3 of the longest hardly counts, while row
   lengths within a factor 4 of each other keep the parity bars. */
/* device pointers: m matched keypoint pairs -> result (R, T, diagnostics). */
erp_status erp_eight_point_find_dev(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* d_kl,
                                    const erp_point2f* d_kr, int32_t m, const erp_ransac_cfg* cfg,
                                    erp_pair_result* d_result, erp_hypothesis* d_hyps,
                                    void* stream);
/* device pointers: the initial_guess ITERATIONS only (no consensus) -> cfg->iters records.
   cfg->offset positions the glibc stream, so iteration block [a, b) of a larger find() is
   reproduced exactly with iters = b - a and offset = base + a*(m-1): the hypothesis-block
   sharding of configs[4] (src/eight_point.cpp:99-127). */
erp_status erp_eight_point_hypotheses_dev(erp_ctx* ctx, int32_t W, int32_t H,
                                          const erp_point2f* d_kl, const erp_point2f* d_kr,
                                          int32_t m, const erp_ransac_cfg* cfg,
                                          erp_hypothesis* d_hyps, void* stream);
/* device pointers: the trimmed-mean consensus (src/eight_point.cpp:129-149) on K Euler vectors
   d_rvec [K][3] with their translations d_tvec [K][3] (R_vec_arr / T_vec_arr order). */
erp_status erp_consensus_dev(erp_ctx* ctx, const float* d_rvec, const float* d_tvec, int32_t K,
                             double trim_lo, double trim_hi, erp_pair_result* d_result,
                             void* stream);
/* device pointers: valid-list compaction (R1 then R2 per record, src/eight_point.cpp:113-126)
   + the consensus over n_hyps initial_guess records d_hyps (e.g. the rank-ordered all-gather of
   hypothesis blocks; records with both flags 0 push nothing, so blocks may be zero-padded);
   m = match_size (only reported in the result). */
erp_status erp_consensus_hyps_dev(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                  int32_t n_hyps, const erp_ransac_cfg* cfg,
                                  erp_pair_result* d_result, void* stream);
/* The same consensus with its K^2 bounds pass split over nshards ranks (configs[4] strong
   scaling): on every rank, with the same merged d_hyps, call _shard_dev (valid-list compaction
   + the bounds of rows [K*shard/nshards, K*(shard+1)/nshards) into d_lb / d_ub / d_bsel, each
   2*n_hyps entries of 8 bytes, zero elsewhere), SUM the three arrays over the ranks (e.g. one
   RCCL all_reduce), then call _finish_dev on the SAME context (select, refine, exact means,
   first-argmin).  The result equals erp_consensus_hyps_dev's. */
erp_status erp_consensus_hyps_shard_dev(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                        int32_t n_hyps, const erp_ransac_cfg* cfg, int32_t shard,
                                        int32_t nshards, double* d_lb, double* d_ub,
                                        int32_t* d_bsel, void* stream);
erp_status erp_consensus_hyps_finish_dev(erp_ctx* ctx, int32_t m, const erp_hypothesis* d_hyps,
                                         int32_t n_hyps, const erp_ransac_cfg* cfg, double* d_lb,
                                         double* d_ub, int32_t* d_bsel, erp_pair_result* d_result,
                                         void* stream);
/* host pointers, synchronous: the drop-in for eight_point::find. */
erp_status erp_eight_point_find(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* h_kl,
                                const erp_point2f* h_kr, int32_t m, const erp_ransac_cfg* cfg,
                                float R_out[3], float T_out[3], erp_pair_result* h_result);
/* host pointers, synchronous: initial_guess on m bearing pairs (m x 3 doubles each), i.e. find
   after the pixel->bearing step (src/eight_point.cpp:87-150).  The bearings need not be unit
   vectors: each side is scaled by an exact power of two into the fixed point's window, and a
   non-finite component gives ERP_INVALID_ARG ("Input domain" above). */
erp_status erp_initial_guess(erp_ctx* ctx, const double* h_bl, const double* h_br, int32_t m,
                             const erp_ransac_cfg* cfg, float R_out[3], float T_out[3],
                             erp_pair_result* h_result);
/* host pointers, synchronous: one eight_point_estimation on m bearing pairs (m x 3 doubles), any
   finite scale (fp64 Gram); a non-finite component gives ERP_INVALID_ARG. */
erp_status erp_eight_point_estimation(erp_ctx* ctx, const double* h_bl, const double* h_br,
                                      int32_t m, erp_hypothesis* h_out);

/* ---- fused batch: match -> gather -> find for every pair ---- */
erp_status erp_pair_batch_run(erp_ctx* ctx, const erp_pair_batch* batch, float ratio,
                              const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                              void* stream);

/* ---- polish: the winner's inlier set and an iterated inlier refit ----
   No reference counterpart; an opt-in extra like erp_ransac_cfg.inlier_thr.  find returns the
   rotation of ONE 25 % random subset (the consensus winner, src/eight_point.cpp:99-149); with
   wrong matches in the list that answer is often degrees off.  The polish says which matches
   are the winner's inliers and refits eight_point_estimation on them, repeated while the inlier
   set grows.  It is a stage behind find: it reads what erp_pair_batch_run /
   erp_eight_point_find_dev wrote and changes none of it; it draws no rand(), so it never
   touches a rand stream.
   Per pair, from its result record (status, M, min_idx, R, T), its `iters` hypothesis records,
   its gathered matched keypoints key_left / key_right, W, H, a threshold thr > 0 and rounds in
   0..8; all arithmetic fp64 unless stated:
   1. Winner.  Rows are pushed R1 then R2 per record (src/eight_point.cpp:113-126); winner_iter
      is the iteration whose record pushed row min_idx, winner_which 0 for R1 and 1 for R2.
   2. Start state.  e_0 = that record's E; R_0, T_0 = the result record's R, T.
   3. Bearings.  l_i, r_i of every match i < M from the pixels, as find computes them
      (src/eight_point.cpp:163-186).
   4. Inlier set.  For a solved vector e: E' = its rank-2 correction (:45-50), S(e) = the
      matches with |l_i^T E' r_i| < thr, the residual in the fixed order given at
      erp_ransac_cfg.inlier_thr (thr widened from float).
   5. Rounds.  S_0 = S(e_0).  For r = 1..rounds:
        stop if |S_{r-1}| < 9 (below 9 rows the reference's thin-SVD rule applies, and such a
        refit returns "valid" rotations that are radians off);
        e_r = eight_point_estimation on the matches of S_{r-1} (the 36 Gram sums in a fixed
        order, the smallest eigenvector, the estimate with the caller's valid_abs);
        the candidates are the valid ones of R1, R2: stop if there is none;
        R_r = the candidate nearer to R_{r-1} by the consensus' float distance (sqrtf of the
        float squared differences; R1 on a tie), which_r = 0 / 1 says which;
        T_r = the estimate's T, negated if (double)T[0] T_{r-1}[0] + .. [1] + .. [2] (left to
        right) < 0;
        S_r = S(e_r); stop and discard the round if |S_r| < |S_{r-1}|;
        otherwise the round is accepted; stop after it if S_r = S_{r-1} as a set (further
        rounds would repeat it).
   6. Outputs.  rounds_done = the accepted rounds; R, T, E = the last accepted state (with
      rounds_done = 0 the winner's R, T and E byte for byte); n_inliers = |S_rounds_done|,
      n_inliers_winner = |S_0|; the mask = S_rounds_done, one byte (1 / 0) per match and 0 from
      M up to key_stride.  So |S_r| never decreases and rounds = 0 gives the winner's set.
   7. A pair whose record status is not ERP_OK gets that status and zeros (record, rounds and
      mask) -- not an error of the call.  An M above key_stride counts as key_stride, a negative
      one as 0 (as erp_match_error_dev); a pair with more than 65535 matches gets
      ERP_INVALID_ARG, one whose min_idx names no row of its records ERP_INTERNAL.
   The outputs of a pair do not depend on the other pairs of the call and are bit-identical
   from run to run.  The stage is not timed by erp_ctx_set_profiling. */
typedef struct erp_polish_round {   /* one accepted round r (1-based) */
    float R[3];
    float T[3];
    int32_t n_fit;       /* |S_{r-1}|: the matches the refit ran on */
    int32_t n_inliers;   /* |S_r| */
    int32_t which;       /* 0: R = the estimate's R1, 1: its R2 */
    int32_t reserved;
    double E[9];         /* e_r, the solved 9-vector (sign arbitrary) */
} erp_polish_round;
typedef struct erp_polish_result {
    float R[3];
    float T[3];
    int32_t status;      /* the pair's erp_status */
    int32_t winner_iter;
    int32_t winner_which;
    int32_t rounds_done;
    int32_t n_inliers;
    int32_t n_inliers_winner;
    double E[9];
} erp_polish_result;
/* device pointers: what a run with out->results, hyps, key_left, key_right wrote (key_stride =
   its max_nq), or one erp_eight_point_find_dev (n_pairs 1, key_stride >= m) */
typedef struct erp_polish_inputs {
    int32_t n_pairs;
    int32_t iters;                  /* records per pair (cfg->iters of the producing call) */
    int64_t key_stride;             /* keypoint slots per pair */
    const erp_point2f* key_left;    /* [n_pairs][key_stride] */
    const erp_point2f* key_right;   /* [n_pairs][key_stride] */
    const int32_t* width;           /* [n_pairs] */
    const int32_t* height;          /* [n_pairs] */
    const erp_pair_result* results; /* [n_pairs] */
    const erp_hypothesis* hyps;     /* [n_pairs][iters] */
} erp_polish_inputs;
/* device pointers, asynchronous on `stream`, no device-to-host copy and no synchronisation:
   one launch, one workgroup per pair, every round inside it.  valid_abs: the producing call's
   cfg->valid_abs.  d_out [n_pairs]; d_rounds [n_pairs][rounds] (may be NULL; records past
   rounds_done are zero); d_mask [n_pairs][key_stride] (may be NULL).  n_pairs == 0: ERP_OK,
   nothing is done.  thr <= 0, rounds outside 0..8, iters < 1 or key_stride < 0:
   ERP_INVALID_ARG before any GPU work.  The call allocates nothing. */
erp_status erp_polish_dev(erp_ctx* ctx, const erp_polish_inputs* in, double valid_abs, float thr,
                          int32_t rounds, erp_polish_result* d_out, erp_polish_round* d_rounds,
                          uint8_t* d_mask, void* stream);
/* host pointers, synchronous: erp_eight_point_find with the hypothesis records kept on the
   device, followed by the polish.  A consuming call on a rand stream exactly as
   erp_eight_point_find is.  h_result, h_polish and h_mask [m] may be NULL.  Returns the find's
   status (h_polish->status repeats it). */
erp_status erp_eight_point_find_polished(erp_ctx* ctx, int32_t W, int32_t H,
                                         const erp_point2f* h_kl, const erp_point2f* h_kr,
                                         int32_t m, const erp_ransac_cfg* cfg, float thr,
                                         int32_t rounds, erp_pair_result* h_result,
                                         erp_polish_result* h_polish, uint8_t* h_mask);

/* ---- winner records: the winning iteration's E without hypothesis records ----
   find returns R and T but not the essential matrix they came from; the per-iteration records
   (out->hyps, 120 B per iteration) carry it, and the lite route exists to avoid exactly their
   traffic.  The winner stage runs behind the consensus, one workgroup per pair: it finds the
   iteration whose record pushed row min_idx (R1 then R2 per record, src/eight_point.cpp:
   113-126) from the run's own validity flags, rebuilds that iteration's Gram from the sampler's
   selection words still in the context's scratch (the Gram is an exact integer sum, so any order
   gives the pipeline's 36 doubles), solves it by the pipeline's own path (thin Jacobi below 9
   rows, inverse iteration, its Jacobi fallback) and writes E: byte for byte erp_hypothesis.E of
   the same run with records.  Before it writes, it re-runs the estimate on that E and compares
   the chosen rotation and T with the result record's R, T byte for byte: any mismatch (or a
   min_idx that names no row) gives the record status ERP_INTERNAL, never a plausible matrix.
   A pair whose result status is not ERP_OK gets that status and zeros.  The stage allocates
   nothing, synchronises nothing, uses no atomics and draws no rand(). */
typedef struct erp_winner {      /* 88 bytes */
    int32_t status;              /* the pair's erp_status; not ERP_OK: the rest is zero */
    int32_t iter;                /* the iteration whose record pushed row min_idx */
    int32_t which;               /* 0: the row is that iteration's R1, 1: its R2 */
    int32_t sample_n;            /* rows of the sample that was re-solved */
    double E[9];                 /* the solved 9-vector of that iteration: byte for byte
                                    erp_hypothesis.E of the same run with records */
} erp_winner;
/* erp_pair_batch_run followed by the winner stage into d_winners [n_pairs] (device, required),
   on the records route when out->hyps is given (or cfg->inlier_thr > 0) and on the lite route
   otherwise; results and every other output are erp_pair_batch_run's.  A consuming call on a
   rand stream exactly as erp_pair_batch_run is.  With erp_ctx_set_graphs on, this call still
   enqueues plainly (kernel by kernel), as erp_pair_batch_run does under stage timing; the
   winner stage is not timed by erp_ctx_set_profiling.  ERP_INVALID_ARG when d_winners is NULL
   or ERP_OPT_DEBUG_STAGES is not -1 (a skipped stage group would leave another call's scratch
   under the re-solve). */
erp_status erp_pair_batch_run_winners(erp_ctx* ctx, const erp_pair_batch* batch, float ratio,
                                      const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                                      erp_winner* d_winners, void* stream);
/* erp_eight_point_find_dev followed by the winner stage: d_hyps may be NULL (the lite route),
   d_winner [1] is required.  ERP_OPT_DEBUG_STAGES as above. */
erp_status erp_eight_point_find_winner_dev(erp_ctx* ctx, int32_t W, int32_t H,
                                           const erp_point2f* d_kl, const erp_point2f* d_kr,
                                           int32_t m, const erp_ransac_cfg* cfg,
                                           erp_pair_result* d_result, erp_hypothesis* d_hyps,
                                           erp_winner* d_winner, void* stream);
/* host pointers, synchronous: erp_eight_point_find plus the winner record (h_winner required;
   R_out, T_out, h_result may be NULL).  Returns the find's status. */
erp_status erp_eight_point_find_winner(erp_ctx* ctx, int32_t W, int32_t H,
                                       const erp_point2f* h_kl, const erp_point2f* h_kr,
                                       int32_t m, const erp_ransac_cfg* cfg, float R_out[3],
                                       float T_out[3], erp_pair_result* h_result,
                                       erp_winner* h_winner);
/* erp_polish_dev with steps 1-2 of its rules taken from winner records: winner_iter,
   winner_which and e_0 are d_winners[p]'s iter, which and E; in->hyps and in->iters are not
   read.  A winner status that is not ERP_OK is handled like a result status that is not ERP_OK
   (step 7; the result's status comes first).  Everything else is erp_polish_dev's: given the
   winners and results of one run, the outputs are byte-identical to erp_polish_dev on that
   run's records. */
erp_status erp_polish_winners_dev(erp_ctx* ctx, const erp_polish_inputs* in,
                                  const erp_winner* d_winners, double valid_abs, float thr,
                                  int32_t rounds, erp_polish_result* d_out,
                                  erp_polish_round* d_rounds, uint8_t* d_mask, void* stream);

/* ---- support-scored winner: the best-supported hypothesis per pair ----
   No reference counterpart; opt-in.  find returns the consensus winner, the rotation nearest
   the trimmed mean of all hypotheses (src/eight_point.cpp:129-149): faithful to the reference,
   and not what a RANSAC user expects, which is the hypothesis most matches agree with.  The
   support stage runs behind the consensus, on the same context, and reads the run's scratch as
   the winner stage does -- on the records route (out->hyps given, or cfg->inlier_thr > 0) and on
   the lite route alike; cfg->inlier_thr may stay 0.  Per pair with result status ERP_OK, a
   threshold thr > 0 (float, widened to double) and the call's cfg (all exact):
   1. e_h = the solved 9-vector of iteration h, byte for byte erp_hypothesis.E of the same run
      with records; E'_h = E_mat_correct(e_h) (src/eight_point.cpp:45-50).
   2. count_h = #{ i < M : |l_i^T E'_h r_i| < thr }, fp64 in the fixed order given at
      erp_ransac_cfg.inlier_thr: for every h exactly what cfg->inlier_thr = thr writes into
      hyps[h].inliers.  Iterations with no valid rotation get a count too.
   3. Scored iterations are those with R1 or R2 valid.  iter = the scored iteration with the
      largest count, the smallest h on ties.  which = its valid rotation; when both are valid, the
      one nearer to the result record's R by the consensus' float distance (sqrtf of the float
      squared differences, src/eight_point.cpp:138-139), R1 on a tie: the polish's rule.
   4. row = the index (iter, which) has in push order (R1 then R2 per iteration, :113-126).
   5. consensus_iter = the iteration that pushed row min_idx; consensus_inliers = its count.
   Before it writes, the stage re-runs the estimate on e_iter and compares the validity flags
   and, byte for byte, the chosen rotation and T with what the run stored for that iteration: a
   mismatch (or a min_idx that names no row) gives the pair ERP_INTERNAL and zeros, never a
   plausible record.  A pair whose result status is not ERP_OK gets that status and zeros.
   When it pays: with minimal samples (cfg->sample_frac chosen for s ~ 10 rows) the best-supported
   hypothesis recovers the pose where the consensus winner is degrees off; with the reference's
   25 % samples every sample of a contaminated list is contaminated and the support winner is
   no better, often worse (INTEGRATION.md has the table).  The stage allocates nothing inside the
   call's enqueue, synchronises nothing, uses no atomics and draws no rand(). */
typedef struct erp_support {     /* 32 bytes */
    int32_t status;              /* the pair's erp_status; not ERP_OK: the rest is zero */
    int32_t iter;                /* the best-supported scored iteration */
    int32_t which;               /* 0: its R1, 1: its R2 (rule 3) */
    int32_t inliers;             /* count_iter */
    int32_t scored;              /* iterations with a valid rotation */
    int32_t consensus_iter;      /* the iteration that pushed row min_idx */
    int32_t consensus_inliers;   /* its count */
    int32_t row;                 /* (iter, which) in R_vec_arr order */
} erp_support;
/* device outputs of the support stage (caller-owned; NULL = not needed) */
typedef struct erp_support_outputs {
    erp_support* support;        /* [n_pairs] (required) */
    erp_winner* winners;         /* [n_pairs] {status, iter, which, sample_n, E = e_iter}: what
                                    erp_polish_winners_dev, erp_pose_select_dev,
                                    erp_match_guided_dev and erp_epipolar_draw_dev take */
    erp_pair_result* results;    /* [n_pairs] the run's records with R and T replaced by that
                                    iteration's chosen rotation and its T (the f32 values the
                                    estimate wrote) and min_idx by row; every other field is
                                    copied: min_dist, near_ties, survivors and binned_rows still
                                    describe the consensus.  A pair that is not ERP_OK: a copy */
    int32_t* counts;             /* [n_pairs][iters] count_h; rows of pairs that are not ERP_OK
                                    are zeros */
} erp_support_outputs;
/* erp_pair_batch_run followed by the support stage; results and every other output of `out` are
   erp_pair_batch_run's.  A consuming call on a rand stream exactly as erp_pair_batch_run is.
   With erp_ctx_set_graphs on, this call still enqueues plainly; the stage is not timed by
   erp_ctx_set_profiling.  ERP_INVALID_ARG when thr <= 0 or not finite, sup or sup->support is
   NULL, or ERP_OPT_DEBUG_STAGES is not -1 (a skipped stage group would leave another call's
   scratch under the stage). */
erp_status erp_pair_batch_run_support(erp_ctx* ctx, const erp_pair_batch* batch, float ratio,
                                      const erp_ransac_cfg* cfg, const erp_batch_outputs* out,
                                      float thr, const erp_support_outputs* sup, void* stream);
/* erp_eight_point_find_dev followed by the support stage (n_pairs = 1): d_hyps may be NULL (the
   lite route).  Arguments as above. */
erp_status erp_eight_point_find_support_dev(erp_ctx* ctx, int32_t W, int32_t H,
                                            const erp_point2f* d_kl, const erp_point2f* d_kr,
                                            int32_t m, const erp_ransac_cfg* cfg,
                                            erp_pair_result* d_result, erp_hypothesis* d_hyps,
                                            float thr, const erp_support_outputs* sup,
                                            void* stream);
/* host pointers, synchronous: erp_eight_point_find plus the support stage.  h_support is
   required; R_out, T_out (the support winner's rotation and T), h_result (find's own record),
   h_winner, h_support_result and h_counts [cfg->iters] may be NULL.  Returns the find's status. */
erp_status erp_eight_point_find_support(erp_ctx* ctx, int32_t W, int32_t H,
                                        const erp_point2f* h_kl, const erp_point2f* h_kr,
                                        int32_t m, const erp_ransac_cfg* cfg, float thr,
                                        float R_out[3], float T_out[3], erp_pair_result* h_result,
                                        erp_support* h_support, erp_winner* h_winner,
                                        erp_pair_result* h_support_result, int32_t* h_counts);

/* ---- pose selection: the cheirality vote over (R1 | R2) x (+t | -t), with depths ----
   No reference counterpart; opt-in.  decomposeEssentialMat gives two rotations and a translation
   of arbitrary sign; the reference keeps whichever rotation has every Euler angle under 1.57 rad
   (src/eight_point.cpp:70-84) and never decides the sign of T, so find's answer is half a pose
   and a rotation above 90 degrees on an axis cannot be returned at all.  This stage makes the
   decision every essential-matrix user expects (OpenCV: recoverPose): it triangulates the
   matches under the four candidates and keeps the one that puts the points in front of both
   cameras -- on the sphere "in front" is a positive depth along both bearings, so all four
   candidates are testable.  R and T of the record are the reference's (R1 | R2, +-t) made
   definite, not new quantities.  It is a stage behind find, the winner records and the polish:
   it reads what they wrote and changes none of it, draws no rand(), allocates nothing,
   synchronises nothing and uses no atomics.
   Per pair, from its result record (status, M, R, T), a solved 9-vector e, its gathered matched
   keypoints, W, H, an optional byte mask, thr and min_sin2 >= 0; all arithmetic fp64, products
   and sums evaluated left to right as written (the library is built with contraction off):
   1. Candidates.  E' = the rank-2 correction of e (:45-50); (R1, R2, t) = decompose_e(E')
      (cv::decomposeEssentialMat).  Candidate k = 2 * which + s has the rotation Rc = which ? R2
      : R1 and the translation tc = s ? -t : t.  The model is the one decomposeEssentialMat
      inverts, E' = [t]x R with the residual l^T E' r:  d_l * l = d_r * (Rc r) + tc,  d_l and d_r
      the depths along the left and the right bearing in units of the baseline.
   2. Per match i < M: l, r = the bearings as find computes them (:163-186).  For each of R1 and
      R2: q = Rc r (q_i = Rc[i][0] r_0 + Rc[i][1] r_1 + Rc[i][2] r_2);  a = l.l, b = l.q,
      c = q.q, lt = l.t, qt = q.t (x.y = x_0 y_0 + x_1 y_1 + x_2 y_2);  det = a*c - b*b (the
      squared sine of the parallax);  d_l = (c*lt - b*qt) / det,  d_r = (b*lt - a*qt) / det.
      Under -t both depths change sign exactly, so they are computed once per rotation.
   3. Voters.  Match i votes if the mask is NULL or mask[i] != 0;  thr <= 0 or
      |l^T E' r| < thr (the residual in the fixed order given at erp_ransac_cfg.inlier_thr, thr
      widened from float);  and, for the rotation in question, det > 0 and det >= min_sin2.  It
      votes for (Rc, +t) if d_l > 0 && d_r > 0 and for (Rc, -t) if d_l < 0 && d_r < 0.  n_voters
      counts the matches that pass the mask and threshold tests and the parallax test for at
      least one rotation.
   4. Selection.  The candidate with the most votes wins, the lowest k on a tie.  n_voters == 0
      gives the pose status ERP_TOO_FEW_POINTS and zeros (n_voters and votes are kept: all 0).
   5. The record erp_pose, below.
   6. Optional outputs: depth (d_l, d_r) under the selected pose (both negated when t_sign is
      -1) for the matches that pass rule 3's tests for the selected rotation, 0 elsewhere;
      front = 1 where the match voted for the selected candidate;  results_out = the result
      records with R and T replaced by the pose's where the POSE's status is ERP_OK, every other
      byte (and every byte of the other records) copied: it feeds erp_rectify_results_dev as it
      is.  depth and front are 0 from M up to key_stride.
   7. Status rules are the polish's step 7: a result status that is not ERP_OK, or a source
      status that is not ERP_OK (the result's comes first), gives that status and zeros -- not an
      error of the call.  An M above key_stride counts as key_stride, a negative one as 0; a
      pair with more than 65535 matches gets ERP_INVALID_ARG.
   8. The outputs of a pair do not depend on the other pairs of the call and are bit-identical
      from run to run.  The stage is not timed by erp_ctx_set_profiling. */
typedef struct erp_pose {        /* 160 bytes */
    int32_t status;      /* the pair's erp_status; not ERP_OK: the rest is zero */
    int32_t which;       /* 0: the selected rotation is decompose_e's R1, 1: its R2 */
    int32_t t_sign;      /* +1: the selected translation is decompose_e's t, -1: -t */
    int32_t n_voters;
    int32_t votes[4];    /* votes[k], k = 2 * which + (t_sign < 0) */
    int32_t rot_agrees;  /* 1: R below equals the result record's R byte for byte */
    int32_t t_flipped;   /* 1: (double)T[0] T_res[0] + .. [1] + .. [2] (left to right) < 0, T_res
                            the result record's T: the selected T is the result's negated */
    float R[3];          /* rot2eular of Rm (XYZ Euler, rad), narrowed */
    float T[3];          /* t, narrowed */
    double Rm[9];        /* the selected rotation matrix, row-major */
    double t[3];         /* the selected translation tc (unit) */
} erp_pose;
/* device pointers.  n_pairs .. results as in erp_polish_inputs.  e: pair p's solved 9-vector is
   the 9 doubles at (char*)e + p * e_stride (8-byte aligned, e_stride a multiple of 8);
   src_status (may be NULL): pair p's int32 source status at (char*)src_status + p *
   src_status_stride.  From winner records: e = &d_winners[0].E, e_stride = 88, src_status =
   &d_winners[0].status, src_status_stride = 88, with a thr > 0; from the polish: e =
   &d_polish[0].E, src_status = &d_polish[0].status, both strides 120, mask = the polish's mask
   and thr <= 0. */
typedef struct erp_pose_inputs {
    int32_t n_pairs;
    int32_t reserved;               /* 0 */
    int64_t key_stride;             /* keypoint (and mask) slots per pair */
    const erp_point2f* key_left;    /* [n_pairs][key_stride] */
    const erp_point2f* key_right;   /* [n_pairs][key_stride] */
    const int32_t* width;           /* [n_pairs] */
    const int32_t* height;          /* [n_pairs] */
    const erp_pair_result* results; /* [n_pairs] */
    const void* e;
    int64_t e_stride;
    const void* src_status;         /* may be NULL */
    int64_t src_status_stride;
    const uint8_t* mask;            /* [n_pairs][key_stride]; may be NULL */
} erp_pose_inputs;
/* device pointers, asynchronous on `stream`, no device-to-host copy and no synchronisation: one
   launch, one workgroup per pair.  d_out [n_pairs]; d_depth [n_pairs][key_stride][2] doubles,
   d_front [n_pairs][key_stride] bytes and d_results_out [n_pairs] may each be NULL (d_results_out
   may be in->results itself).  n_pairs == 0: ERP_OK, nothing is done.  min_sin2 < 0, a NaN thr
   or min_sin2, key_stride < 0 or a misaligned e: ERP_INVALID_ARG before any GPU work.  The call
   allocates nothing. */
erp_status erp_pose_select_dev(erp_ctx* ctx, const erp_pose_inputs* in, float thr, double min_sin2,
                               erp_pose* d_out, double* d_depth, uint8_t* d_front,
                               erp_pair_result* d_results_out, void* stream);
/* host pointers, synchronous: erp_eight_point_find with its winner record on the lite route,
   then erp_polish_winners_dev with thr (> 0) and rounds (0..8), then the selection on the
   polish's E and mask (no residual test of its own: the mask is the polish's inlier set).  A
   consuming call on a rand stream exactly as erp_eight_point_find is; a call that fails on thr,
   rounds or min_sin2 consumes nothing.  h_result, h_polish, h_pose, h_mask [m], h_depth [m][2]
   and h_front [m] may be NULL.  Returns the find's status (h_pose->status is the pose's). */
erp_status erp_eight_point_find_posed(erp_ctx* ctx, int32_t W, int32_t H, const erp_point2f* h_kl,
                                      const erp_point2f* h_kr, int32_t m,
                                      const erp_ransac_cfg* cfg, float thr, int32_t rounds,
                                      double min_sin2, erp_pair_result* h_result,
                                      erp_polish_result* h_polish, erp_pose* h_pose,
                                      uint8_t* h_mask, double* h_depth, uint8_t* h_front);

/* ---- guided matching: the descriptors rematched inside the epipolar band of a solved E ----
   No reference counterpart; opt-in.  match_two_image keeps a query when d0 < 0.3 * d1 over ALL
   train rows (src/feature_matcher.cpp:42-59): nothing but descriptor distance is known before the
   geometry is.  Once an essential matrix is solved, the candidates of a query can be restricted
   to the train keypoints near its epipolar line, and a much looser ratio is safe there.  The
   stage runs behind find, the winner records and the polish: it reads a packed batch
   (erp_pair_batch), result records and a solved 9-vector per pair and changes none of them.
   Per pair p of the batch (dim 64; nq = its left rows, nt = its right rows), from its result
   record, e at (e, e_stride) and an optional source status at (src_status, src_status_stride),
   both addressed as in erp_pose_inputs, and erp_guided_cfg; arithmetic as stated (the library is
   built with contraction off):
   1. E' = the rank-2 correction of e (src/eight_point.cpp:45-50).  l_i, i < nq, and r_j,
      j < nt, are the bearings of the left and right keypoints as find computes them
      (:163-186).
   2. Gate.  G_i = { j : |l_i^T E' r_j| < thr }, the fp64 residual in the fixed order given at
      erp_ransac_cfg.inlier_thr, thr widened from float.  A NaN residual (a non-finite keypoint)
      is not gated and changes no status.  A guided match is therefore an inlier of the polish's
      rule 4 at the same thr and E, bit for bit.
   3. Distances.  e(i, j) = the squared distance in the flann::L2<float> order (the matcher's),
      d = sqrtf(e).  j0 = the j of G_i with the smallest e, the lowest j among equal e;
      d0 = d(i, j0); d1 = the smallest d over G_i without j0 (it may equal d0), +inf when
      |G_i| = 1.
   4. Query i is accepted when |G_i| >= 1, d0 < ratio * d1 (the float product of the matcher's
      ratio test; true against +inf) and (max_dist <= 0 or d0 < max_dist).
   5. unique != 0: among the accepted queries with the same j0 only the one with the smallest d0
      stays, the lowest i among equal d0.
   6. Outputs, each optional but count: count[p] = M_g, the queries that stay;  matches
      [n_pairs][max_nq] in ascending queryIdx (pair-local indices, imgIdx 0, distance = d0);
      key_left / key_right [n_pairs][max_nq], the keypoints of those matches;  gated [n_pairs]
      (int64) = the sum over i of |G_i|;  results_out [n_pairs] = the result record with M
      replaced by M_g and every other byte copied (it may be the input itself);  winners_out
      [n_pairs] = an erp_winner with the pair's status, iter -1, which 0, sample_n 0 and E = e.
      With results_out, winners_out and the gathered keys, erp_polish_winners_dev and
      erp_pose_select_dev run on the guided list unchanged (the polish only copies iter and
      which).  matches and keys are zero from M_g up to max_nq.
   7. Status rules are the pose selection's rule 7: a result status that is not ERP_OK, or a
      source status that is not ERP_OK (the result's comes first), gives count 0, gated 0, zero
      matches and keys, M = 0 in results_out and a winners_out record with that status and zeros
      -- not an error of the call.  nq = 0 or nt = 0 gives count 0 with ERP_OK.  dim != 64,
      thr <= 0 or NaN, ratio <= 0 or NaN, a NaN max_dist, a misaligned e or max_nq > 65535 (as
      erp_pair_batch_run refuses it) give ERP_INVALID_ARG before any GPU work.
   8. The outputs of a pair do not depend on the other pairs of the call and are bit-identical
      from run to run: the only atomics are a 64-bit integer min (rule 5) and a 64-bit integer
      add (gated), whose results do not depend on the order.  The stage draws no rand(), never
      touches a rand stream and synchronises nothing; it is not timed by erp_ctx_set_profiling.
   Consequence: |l^T E' r| <= 0.7072 for unit bearings and a unit-norm e, so thr = 1 gates
   every finite pair (i, j); with unique = 0 and max_dist = 0 the list is then, for nt >= 2,
   erp_match_knn2_ratio's at the same ratio, bit for bit. */
typedef struct erp_guided_cfg {
    float thr;           /* > 0: the gate, as erp_ransac_cfg.inlier_thr */
    float ratio;         /* > 0: d0 < ratio * d1 */
    float max_dist;      /* <= 0: off; otherwise d0 < max_dist */
    int32_t unique;      /* != 0: rule 5 */
} erp_guided_cfg;
/* device pointers.  batch: as erp_pair_batch_run reads it (max_nt bounds the right rows per
   pair).  results may be NULL: every pair then counts as ERP_OK (and results_out must be NULL).
   e / src_status: as in erp_pose_inputs (from winner records: &d_winners[0].E and .status, both
   strides 88; from the polish: &d_polish[0].E and .status, both strides 120). */
typedef struct erp_guided_inputs {
    erp_pair_batch batch;
    const erp_pair_result* results; /* [n_pairs]; may be NULL */
    const void* e;
    int64_t e_stride;
    const void* src_status;         /* may be NULL */
    int64_t src_status_stride;
} erp_guided_inputs;
typedef struct erp_guided_outputs {
    int32_t* count;                 /* [n_pairs] (required) */
    erp_dmatch* matches;            /* [n_pairs][max_nq] */
    erp_point2f* key_left;          /* [n_pairs][max_nq] */
    erp_point2f* key_right;         /* [n_pairs][max_nq] */
    int64_t* gated;                 /* [n_pairs] */
    erp_pair_result* results_out;   /* [n_pairs] */
    erp_winner* winners_out;        /* [n_pairs] */
} erp_guided_outputs;
/* device pointers, asynchronous on `stream`, no device-to-host copy and no synchronisation:
   three launches (bearings and E', gate and top-2, compaction).  n_pairs == 0: ERP_OK, nothing
   is done.  The context's scratch for the stage (per query 16 bytes, per train row 48) grows on
   the first call of a shape and is reused afterwards (erp_ctx_reserve does not cover it). */
erp_status erp_match_guided_dev(erp_ctx* ctx, const erp_guided_inputs* in,
                                const erp_guided_cfg* cfg, const erp_guided_outputs* out,
                                void* stream);
/* host pointers, synchronous, one pair, no result record: h_desc1 [n1][64], h_desc2 [n2][64],
   h_kp1 [n1], h_kp2 [n2], E the solved 9-vector -> h_out [n1] (the first *h_count are valid).
   n1 > 65535, W or H <= 0: ERP_INVALID_ARG. */
erp_status erp_match_guided(erp_ctx* ctx, const float* h_desc1, int32_t n1, const float* h_desc2,
                            int32_t n2, const erp_point2f* h_kp1, const erp_point2f* h_kp2,
                            int32_t W, int32_t H, const double E[9], const erp_guided_cfg* cfg,
                            erp_dmatch* h_out, int32_t* h_count);

/* ---- ERP remaps around the hot path ----
   Images are 8-bit 3-channel (CV_8UC3, BGR) H x W x 3, row-major, device pointers.  Output
   pixels whose inverse-warped source falls outside the image are NOT written (the reference
   leaves them uninitialised): pre-fill the outputs. */
/* spherical_surf::crop_rotated_image(pitch, im) (src/spherical_surf.cpp:16-48): the central
   H/4 rows of the image rotated by pitch degrees about Y -> d_out (H/4) x W x 3. */
erp_status erp_crop_rotated_image_dev(erp_ctx* ctx, const uint8_t* d_im, int32_t W, int32_t H,
                                      float pitch_deg, uint8_t* d_out, void* stream);
/* the four bands of spherical_surf::do_all (src/spherical_surf.cpp:77-93) for n_images images
   (contiguous, each H x W x 3): d_bands [n][4][H/4][W][3] = crop(45), rows [3H/8, 3H/8 + H/4),
   crop(-45), crop(-90). */
erp_status erp_spherical_bands_dev(erp_ctx* ctx, const uint8_t* d_ims, int32_t n_images,
                                   int32_t W, int32_t H, uint8_t* d_bands, void* stream);
/* spherical_surf::rotate_keypoint(pitch, key, width, height) (src/spherical_surf.cpp:50-63),
   in place on n keypoints (pt.x, pt.y). */
erp_status erp_rotate_keypoints_dev(erp_ctx* ctx, erp_point2f* d_kp, int32_t n, float pitch_deg,
                                    int32_t W, int32_t H, void* stream);
/* do_all's keypoint un-rotation (src/spherical_surf.cpp:120-133) on the band keypoints
   concatenated in band order n0, n1, n2, n3 (counts[4]), in place: the result is the
   left_key_tmp / right_key_tmp index space of the matcher (:136-144). */
erp_status erp_unrotate_band_keypoints_dev(erp_ctx* ctx, erp_point2f* d_kp,
                                           const int32_t counts[4], int32_t W, int32_t H,
                                           void* stream);
/* erp_rotation::rotate_image(im, rot_mat) (src/erp_rotation.cpp:94-122). */
erp_status erp_rotate_image_dev(erp_ctx* ctx, const uint8_t* d_im, int32_t W, int32_t H,
                                const double rot_mat[9], uint8_t* d_out, void* stream);
/* rectify(im_left, im_right, R_vec, T_vec) (src/automatic.cpp:66-79): both rotate_image calls
   in one launch. */
erp_status erp_rectify_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int32_t W,
                           int32_t H, const double rot_vec[3], const double t_vec[3],
                           uint8_t* d_left_out, uint8_t* d_right_out, void* stream);
/* the vertical view of src/automatic.cpp:148-151: rotate_image by eular2rot(RAD(89.999), 0, 0)
   .inv(), then cv::rotate(ROTATE_90_CLOCKWISE), fused -> d_out W x H x 3 (W rows). */
erp_status erp_vertical_rotate_dev(erp_ctx* ctx, const uint8_t* d_im, int32_t W, int32_t H,
                                   uint8_t* d_out, void* stream);
/* ---- batched rectification: what src/automatic.cpp:138-160 produces, for many pairs ----
   Images lie one after the other in their stacks ([n][H][W][3] in, [n][W][H][3] vertical views).
   `fill` in 0..255 pre-fills every output with that byte; -1 leaves the outputs as the caller
   set them (pixels without a source stay unwritten, as above).  Outputs must not overlap the
   inputs or each other.  n == 0 / n_pairs == 0: ERP_OK, nothing is done. */
/* erp_vertical_rotate_dev for n images: d_ims [n][H][W][3] -> d_out [n][W][H][3], byte for
   byte what n calls give.  The vertical view applies one fixed matrix, so the source pixel of
   an output pixel is computed once and copied for all n images (ERP_OPT_VERTICAL_SHARED).
   Asynchronous on `stream`. */
erp_status erp_vertical_rotate_batch_dev(erp_ctx* ctx, const uint8_t* d_ims, int32_t n, int32_t W,
                                         int32_t H, int32_t fill, uint8_t* d_out, void* stream);
/* caller-owned device outputs of the batched rectification */
typedef struct erp_rectify_outputs {
    uint8_t* left_rect;         /* [n_pairs][H][W][3] (required) */
    uint8_t* right_rect;        /* [n_pairs][H][W][3] (required) */
    uint8_t* left_vertical;     /* [n_pairs][W][H][3]; both NULL = no vertical stage */
    uint8_t* right_vertical;    /* [n_pairs][W][H][3] */
    int32_t* done;              /* [n_pairs] 1 = the pair's images were written, 0 = not; may be
                                   NULL */
} erp_rectify_outputs;
/* rectify (src/automatic.cpp:66-79) of n_pairs pairs d_left / d_right [n_pairs][H][W][3], then
   the two vertical views of every pair (:146-153).  h_rot_vec / h_t_vec [n_pairs][3] doubles on
   the HOST (read before the call returns) go through erp_rectify_matrices per pair; a pair it
   rejects, or whose h_skip entry ([n_pairs] int32 on the host, may be NULL) is non-zero, is not
   remapped: done = 0 and its rectified images stay at `fill` -- not an error of the call.  The
   vertical stage runs over all 2 n_pairs rectified images, so such a pair's vertical views are
   those of its fill-valued (or, with fill = -1, caller-set) rectified images.  Per pair the
   bytes are erp_rectify_dev's and erp_vertical_rotate_dev's.  Asynchronous on `stream`. */
erp_status erp_rectify_batch_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                                 int32_t n_pairs, int32_t W, int32_t H, const double* h_rot_vec,
                                 const double* h_t_vec, const int32_t* h_skip, int32_t fill,
                                 const erp_rectify_outputs* outputs, void* stream);
/* erp_rectify_batch_dev with the poses of device records d_results [n_pairs] (what
   erp_pair_batch_run / erp_image_pairs_run write): R and T widened float -> double as
   src/automatic.cpp:128-129 does (erp_rectify_matrices_results); a pair whose status is not
   ERP_OK is skipped.  NOT graph-capturable and not asynchronous: one device-to-host copy of the
   records and one synchronisation of `stream` precede the launches. */
erp_status erp_rectify_results_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                                   int32_t n_pairs, int32_t W, int32_t H,
                                   const erp_pair_result* d_results, int32_t fill,
                                   const erp_rectify_outputs* outputs, void* stream);

/* ---- dense stereo on row-rectified views: census + 4- or 8-path SGM (no reference counterpart) --
   The vertical views of erp_rectify_outputs are what this is for: rectify turns the baseline
   onto (0, -1, 0), the 89.999-degree turn about x puts both epipoles on the poles and the
   90-degree rotation makes every meridian -- one epipolar half-plane -- a row, so that a scene
   point lies on the same row of both [W rows][H columns] views and stereo is a 1-D search
   along rows (rows = W, cols = H, wrap_rows = 1: the row index is longitude and periodic).
   The call works on any pair of row-rectified 8-bit images.

   Rules.  Everything is integer arithmetic except the depth, so a caller can restate the
   output bit for bit (tests/stereo_ref.py does).  Pixel (y, x) of both images belongs to row y;
   D = n_disp.
   1. Gray.  channels == 3: (b*1868 + g*9617 + r*4899 + 8192) >> 14 on the bytes b, g, r in that
      order (SURF's gray conversion); channels == 1: the byte.
   2. Census.  Window 9 wide, 7 tall; its neighbours in row-major order, dy = -3..3, dx = -4..4,
      the centre skipped: 62 bits.  Bit k (LSB first) = gray(neighbour k) < gray(centre).
      Columns clamp to [0, cols-1].  Rows wrap modulo `rows` (any rows >= 1, also below 7) when
      wrap_rows is set and clamp to [0, rows-1] otherwise.
   3. Cost.  For d in [0, D): xr = x - d_min - d; c(y,x,d) = popcount(cenL(y,x) ^ cenR(y,xr))
      when 0 <= xr < cols, else 63.
   4. Aggregation.  Four paths r: left to right, right to left, top to bottom, bottom to top;
      none wraps.  The first pixel of a path has L_r = c.  After it, with q the previous pixel on
      the path and m = min_k L_r(q,k),
        L_r(p,d) = c(p,d) + min(L_r(q,d), L_r(q,d-1) + p1, L_r(q,d+1) + p1, m + p2) - m,
      a neighbour d-1 or d+1 outside [0, D) left out.  S = the sum of the four L_r, uint16
      (L_r <= 63 + p2, so S <= 1272).
   4b. The diagonal paths (erp_stereo_params_ex.n_paths == 8).  Four more paths r with the steps
      (dy, dx) = (+1, +1), (-1, -1), (+1, -1), (-1, +1).  The previous pixel of p = (y, x) on
      path r is q = (y - dy, x - dx).  When q's column is outside [0, cols), p is the first pixel
      of its path: L_r = c.  When q's row is outside [0, rows): with wrap_rows == 1 the row is
      taken modulo `rows` (any rows >= 1; at rows == 1 a diagonal is the row path), with
      wrap_rows == 0 p is a first pixel.  Otherwise rule 4's recurrence, unchanged.  S = the sum
      of all eight L_r, still uint16: S <= 8 * (63 + p2) = 2544.  The four paths of rule 4 still
      do not wrap.
   5. Winner and sub-pixel.  d* = the first argmin over d of S(y,x,.).  a = S[d*-1],
      b = S[d*+1], c = S[d*], den = a + b - 2c.  off = 0 when d* is 0 or D-1 or den <= 0, else
      off = floor(((a - b)*16 + den) / (2*den)) (floor division on signed integers).
      disp16 = 16*(d_min + d*) + off.
   6. Right disparity and left-right check.  dR(y,xr) = the first argmin over d of
      S(y, xr + d_min + d, d) over the d whose column xr + d_min + d is in [0, cols).  Pixel
      (y,x) is invalid (ERP_STEREO_INVALID) when its xr = x - d_min - d* is outside [0, cols),
      or when lr_max >= 0 and abs(d* - dR(y,xr)) > lr_max.
   6b. Uniqueness (erp_stereo_params_ex.uniqueness > 0), after rules 5 and 6.  Pixel (y,x) is
      also invalid when some d with abs(d - d*) > 1 has
      S(y,x,d) * (100 - uniqueness) < S(y,x,d*) * 100.  dR does not depend on it.
   7. Depth (optional), the left camera's, in units of |t|, meant for vertical views, where a
      row runs from pole to pole; the pixel-to-angle rule is the reference's pi * i / H
      (src/erp_rotation.cpp:68; no half-pixel offset).  thL = pi*x/cols,
      thR = pi*(x - disp16/16.0)/cols, depth = sin(thR) / abs(sin(thL - thR)), evaluated in
      fp64 in exactly that order (M_PI * x, then / cols) and stored as float: the sine rule on
      the triangle (left centre, right centre, point), whose angle at the point is
      abs(thL - thR) and whose interior angle at the right centre has sine sin(thR) whichever
      pole the baseline points to.  +inf where disp16 == 0, NaN where the
      pixel is invalid.

   p1 = 8 and p2 = 64 are starting values: nobody has tuned them on real views yet. */
#define ERP_STEREO_INVALID (-32768)
typedef struct erp_stereo_params {
    int32_t d_min;      /* first disparity searched (signed); default 0 */
    int32_t n_disp;     /* D: a multiple of 16 in 16..256, abs(d_min) + D <= 2047; default 64 */
    int32_t p1;         /* 0 <= p1 <= p2 <= 255; default 8 */
    int32_t p2;         /* default 64 */
    int32_t lr_max;     /* whole pixels; -1 disables the left-right check; default 1 */
    int32_t wrap_rows;  /* 0 or 1; 1 for vertical views; default 0 */
    int32_t channels;   /* 1 or 3; default 3 */
} erp_stereo_params;
void erp_stereo_params_default(erp_stereo_params* p);
/* d_left / d_right [n_pairs][rows][cols][channels] uint8 -> d_disp16 [n_pairs][rows][cols]
   int16, the left image's disparity in 1/16 pixel (ERP_STEREO_INVALID where rejected), and
   d_depth [n_pairs][rows][cols] float (may be NULL).  Device pointers; asynchronous on
   `stream`; deterministic (no atomics, no floating-point sums).  The census words, the S
   volume (rows * cols * D * 2 bytes per pair) and the winners live in the context's grow-only
   scratch, sized for a chunk of pairs at a time: as many pairs as fit ERP_OPT_STEREO_CHUNK_MB
   of S volume (default 1024 MiB), at least one; the chunks run one after the other on
   `stream` and every chunk size gives the same bytes.
   n_pairs == 0: ERP_OK, nothing is done.  Before any launch, ERP_INVALID_ARG for: a NULL ctx,
   params, d_left, d_right or d_disp16, n_pairs < 0, rows < 1, cols < 1, rows * cols > 2^30,
   or a parameter outside the rules of the table above. */
erp_status erp_stereo_rows_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                               int32_t n_pairs, int32_t rows, int32_t cols,
                               const erp_stereo_params* params, int16_t* d_disp16,
                               float* d_depth, void* stream);
/* The same call with rules 4b and 6b.  erp_stereo_params stays as it is; the extension carries
   it.  With the defaults (4 paths, no uniqueness test) the output is erp_stereo_rows_dev's byte
   for byte: that call is this one with them.  The scratch, the chunks and the S volume's size
   are the same; the diagonal paths add two launches per chunk, the uniqueness test none.
   Asynchronous and deterministic like erp_stereo_rows_dev.  Its argument checks, plus
   ERP_INVALID_ARG before any launch for n_paths not 4 or 8, uniqueness outside 0..99 or a
   non-zero reserved field. */
typedef struct erp_stereo_params_ex {
    erp_stereo_params base;
    int32_t n_paths;      /* 4 or 8; default 4 */
    int32_t uniqueness;   /* percent, 0..99; 0 disables; default 0 */
    int32_t reserved[2];  /* must be 0 */
} erp_stereo_params_ex;
void erp_stereo_params_ex_default(erp_stereo_params_ex* p);   /* base = erp_stereo_params_default */
erp_status erp_stereo_rows_ex_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                                  int32_t n_pairs, int32_t rows, int32_t cols,
                                  const erp_stereo_params_ex* params, int16_t* d_disp16,
                                  float* d_depth, void* stream);

/* ---- SURF: feature_matcher::detect_key_point + comput_descriptor
   (src/feature_matcher.cpp:26-40) with xfeatures2d::SURF::create() defaults ---- */
typedef struct erp_keypoint {   /* cv::KeyPoint layout */
    float x, y;                 /* pt */
    float size, angle, response;
    int32_t octave, class_id;
} erp_keypoint;
typedef struct erp_surf_params {
    double hessian_threshold;   /* 100 */
    int32_t n_octaves;          /* 4 */
    int32_t n_octave_layers;    /* 3 */
    int32_t extended;           /* 0 (64-D; 1 is not supported) */
    int32_t upright;            /* 0 (1 is not supported) */
} erp_surf_params;
void erp_surf_params_default(erp_surf_params* p);
/* n_images images of H x W (channels 1 = gray, 3 = BGR), contiguous, device pointers ->
   per image up to max_kp keypoints [n][max_kp] in OpenCV's KeypointGreater order (descending
   response) and their unit 64-D descriptors [n][max_kp][64]; d_count[n] = keypoints found, or
   -(needed) when max_kp was too small (rerun larger).  Enqueued on `stream`; synchronises
   it once inside (the detected counts size the descriptor pass). */
erp_status erp_surf_detect_compute_dev(erp_ctx* ctx, const uint8_t* d_images, int32_t n_images,
                                       int32_t W, int32_t H, int32_t channels,
                                       const erp_surf_params* params, int32_t max_kp,
                                       erp_keypoint* d_kp, float* d_desc, int32_t* d_count,
                                       void* stream);

/* ---- batched do_all: ERP image pairs -> the packed batch erp_pair_batch_run consumes ----
   spherical_surf::do_all (src/spherical_surf.cpp:65-179) up to the match, for many pairs at
   once and without leaving the device: bands (:77-93) -> SURF on every band (:96-118) ->
   keypoint un-rotation + concatenation n0..n3 (:120-150), written straight into the ragged
   layout of erp_pair_batch. */
/* caller-owned device outputs of the pack step; cap_l / cap_r = rows desc_l, kp_l / desc_r,
   kp_r can hold (rows at or past a capacity are not written).  desc_l / desc_r are 16-byte
   aligned. */
typedef struct erp_packed_pairs {
    float* desc_l;              /* [cap_l][64] */
    float* desc_r;              /* [cap_r][64] */
    erp_point2f* kp_l;          /* [cap_l] un-rotated ERP pixels */
    erp_point2f* kp_r;          /* [cap_r] */
    int64_t* off_l;             /* [n_pairs+1] */
    int64_t* off_r;             /* [n_pairs+1] */
    int32_t* width;             /* [n_pairs] */
    int32_t* height;            /* [n_pairs] */
    int32_t* band_counts;       /* [n_pairs][2][4] keypoints per side and band; may be NULL */
    int64_t cap_l;
    int64_t cap_r;
} erp_packed_pairs;
/* what the host learns from erp_image_pairs_features_dev / erp_image_pairs_run */
typedef struct erp_image_batch_info {
    int32_t need_kp;            /* largest raw keypoint count of any band */
    int32_t max_nq;             /* largest left / right row count of any pair */
    int32_t max_nt;
    int32_t groups;             /* groups of pairs the call went through */
    int32_t fits;               /* 1: the outputs are complete.  0: need_kp > max_kp, or rows_l >
                                   cap_l, or rows_r > cap_r: the outputs are unspecified; rerun
                                   with max_kp >= need_kp and capacities >= rows_l / rows_r (a
                                   band that overflowed max_kp contributes no rows to these) */
    int32_t reserved;
    int64_t rows_l;             /* total rows of each side */
    int64_t rows_r;
} erp_image_batch_info;
/* The pack step alone.  d_kp [8 n_pairs][max_kp], d_desc [8 n_pairs][max_kp][64], d_count
   [8 n_pairs] as erp_surf_detect_compute_dev writes them for the band images in the order
   [pair][side left, right][band n0..n3] of W x H ERP images (bands H/4 x W).  Per side and pair
   the rows of bands n0, n1, n2, n3 are concatenated (a count outside [0, max_kp] is clamped
   into it; rows at or past a count are never read), descriptors copied, keypoints un-rotated
   as erp_unrotate_band_keypoints_dev does, pairs appended one after another: out->off_l[p] is
   the first left row of pair p, off_l[n_pairs] the total.  Asynchronous on `stream`. */
erp_status erp_pack_band_features_dev(erp_ctx* ctx, const erp_keypoint* d_kp, const float* d_desc,
                                      const int32_t* d_count, int32_t n_pairs, int32_t max_kp,
                                      int32_t W, int32_t H, const erp_packed_pairs* out,
                                      void* stream);
/* d_left / d_right [n_pairs][H][W][3] (BGR, one size per call) -> the packed batch.  The band
   canvases are pre-filled with the byte `fill` (0 in the reference's Mat::zeros sense; the
   remap leaves out-of-image pixels unwritten); max_kp = keypoint slots per band.  The pairs
   go through in groups (bands, SURF on the group's 8 g bands, pack) so that SURF's scratch
   stays within a fixed budget; max_group_pairs > 0 sets the group size, 0 = the largest that
   fits the budget.  NOT graph-capturable and not asynchronous: the call synchronises `stream`
   a fixed few times per group (SURF's counts) and once at the end (the totals for *info),
   never per pair.  Overflow is reported in info->fits with status ERP_OK. */
erp_status erp_image_pairs_features_dev(erp_ctx* ctx, const uint8_t* d_left,
                                        const uint8_t* d_right, int32_t n_pairs, int32_t W,
                                        int32_t H, const erp_surf_params* params, int32_t max_kp,
                                        int32_t fill, int32_t max_group_pairs,
                                        const erp_packed_pairs* out, erp_image_batch_info* info,
                                        void* stream);
/* erp_image_pairs_features_dev followed, when info->fits and n_pairs > 0, by
   erp_pair_batch_run on the packed batch (dim 64, info's max_nq / max_nt): what
   src/automatic.cpp:117-126 runs per pair, from images to R, T.  Inherits both calls' limits:
   not graph-capturable; a pair with more than 65535 left rows gives ERP_INVALID_ARG (info is
   filled first, so max_nq shows why). */
erp_status erp_image_pairs_run(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                               int32_t n_pairs, int32_t W, int32_t H,
                               const erp_surf_params* params, int32_t max_kp, int32_t fill,
                               int32_t max_group_pairs, const erp_packed_pairs* packed,
                               float ratio, const erp_ransac_cfg* cfg,
                               const erp_batch_outputs* out, erp_image_batch_info* info,
                               void* stream);

/* ---- rotation sweep: one left image against one right base image under a list of poses ----
   What the reference's experiment drivers run per pose (one_image_test/main.cpp:73-145,
   two_synthesis_image_test/main.cpp:80-141, two_real_image_test/main.cpp:169-230):
       rot_mat = eular2rot(rot_vec);  im2 = rotate_image(im_right, rot_mat.inv());
       do_all(im_left, im2, ...);  [the match error];  eight_point::find(...)
   for n_poses poses in one call.  A pose is the driver's rot_mat: h_rot_mat [n_poses][9],
   row-major 3x3 doubles on the HOST, as erp_eular2rot gives them (read before the call
   returns).  Per pose the library forms rot_mat_inv = erp_inv3(rot_mat) and rotates the right
   base image as erp_rotate_image_dev(.., rot_mat_inv, ..) does, so the matrix the remap applies
   is inv3(inv3(rot_mat)) (rotate_image inverts its argument, src/erp_rotation.cpp:103).  A pose
   either inversion finds singular gives ERP_INVALID_ARG before any GPU work.
   The left image's bands and SURF are computed once per call, and only one group's rotated
   right images exist at a time (in context scratch), so the pose count is bounded by the
   packed outputs alone. */
/* The features stage.  d_left, d_right_base: one H x W x 3 image each.  The result is the packed
   batch erp_image_pairs_features_dev writes for n_poses pairs whose left image is d_left and
   whose right image p is rotate_image(right_base, inv3(rot_mat[p])) on a canvas pre-filled with
   `fill` -- byte for byte, *info included (groups apart: it counts this call's groups of
   poses).  Every pair's left rows are the left image's: off_l[p] = p * n_left, band_counts[p][0]
   the left counts; need_kp covers the left bands too.  max_kp, fill (canvases of the rotated
   images and of the bands), max_group_pairs (poses per group, 0 = the largest that fits the
   budget, at most 8), the overflow convention (info->fits with ERP_OK) and the limits -- not
   graph-capturable, synchronises `stream` a fixed few times per group -- are
   erp_image_pairs_features_dev's. */
erp_status erp_image_sweep_features_dev(erp_ctx* ctx, const uint8_t* d_left,
                                        const uint8_t* d_right_base, int32_t n_poses,
                                        const double* h_rot_mat, int32_t W, int32_t H,
                                        const erp_surf_params* params, int32_t max_kp,
                                        int32_t fill, int32_t max_group_pairs,
                                        const erp_packed_pairs* out, erp_image_batch_info* info,
                                        void* stream);
/* erp_image_sweep_features_dev followed, when info->fits and n_poses > 0, by erp_pair_batch_run
   on the packed batch (as erp_image_pairs_run) and, when d_match_error != NULL, by the match
   error of every pose into d_match_error [n_poses] (device).  With a rand stream attached to
   the context the poses draw from it one after the other, as erp_pair_batch_run's pairs do.
   The matched keypoints the match error reads go to out->key_left / key_right where the caller
   gave them (they keep their meaning: [n_poses][info->max_nq]) and to context scratch where
   not.  When info->fits is 0 nothing past the features stage ran (ERP_OK: rerun larger). */
erp_status erp_image_sweep_run(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right_base,
                               int32_t n_poses, const double* h_rot_mat, int32_t W, int32_t H,
                               const erp_surf_params* params, int32_t max_kp, int32_t fill,
                               int32_t max_group_pairs, const erp_packed_pairs* packed,
                               float ratio, const erp_ransac_cfg* cfg,
                               const erp_batch_outputs* out, double* d_match_error,
                               erp_image_batch_info* info, void* stream);
/* The match error alone (one_image_test/main.cpp:115-129 with degree_error :27-50), device
   keypoints, asynchronous on `stream`.  Pair p's matches are d_key_left / d_key_right
   [p * key_stride + i], i < M_p = d_m[p * m_stride] (m_stride in int32 units, >= 1, so
   &results[0].M with sizeof(erp_pair_result) / 4 reads a batch's records; a negative count is
   0, one above key_stride is key_stride); h_rot_mat [n_pairs][9] on the host is each pair's
   pose rot_mat -- applied itself, not its inverse.  Per match, in double:
       (r, c)  = rotate_pixel((int)key_left.y, (int)key_left.x, rot_mat)   (x86 truncation)
       v1      = Point2f((float)c, (float)r),  v2 = key_right
       angles  = M_PI * y / H,  2 * M_PI * x / W      (the float coordinate widened)
       vec     = (sin a cos b, sin a sin b, cos a)    (:35-41, not OMAF's signs)
       product = v1[0] v2[0] + v1[1] v2[1] + v1[2] v2[2]   (left to right, no FMA)
       error   = product < 1 ? acos(product) : 0
   d_out[p] = (the errors added one after the other in match order, from 0.0) / M_p in radians
   (the driver prints it as "degree"); NaN for M_p = 0, as the reference's 0.0 / 0.  The order
   of the sum is fixed, so the result is bit-identical from run to run; sin / cos / acos are
   the device library's (a few ulp from glibc's: <= 1e-7 rad on the mean). */
erp_status erp_match_error_dev(erp_ctx* ctx, const erp_point2f* d_key_left,
                               const erp_point2f* d_key_right, int64_t key_stride,
                               const int32_t* d_m, int64_t m_stride, int32_t n_pairs,
                               const double* h_rot_mat, int32_t W, int32_t H, double* d_out,
                               void* stream);

/* ---- visual outputs, device images ---- */
/* epipolar_tool (src/epipolar_tool.hpp / .cpp:7-71, constructor + draw_epipole :74-128): n_key
   (<= 7, the reference's color_set) of the m matched pairs (host keypoints, ERP pixels of an
   im_width x im_height image) chosen as the first n_key of std::random_shuffle(iota(m)) on the
   glibc rand() stream at (seed, offset) (the process-global rand() state: 1 / 0 in a fresh
   process); on an out_width x out_height CV_8UC3 canvas d_out (written whole) the pixels p with
   |l^T E p| < 0.002 for a chosen left bearing l get that key's colour and 11 x 11 dots mark the
   chosen right keypoints (resized).  E: row-major 3x3 (test_E_mat).  The reference's OpenMP
   loop races on overlapping writes; here the sequential order of its loop decides: a pixel
   shows the last key whose dot covers it, else the last key whose curve passes, else 0 (the
   corner pixel (H-1, W-1) interleaves curve k and dot k in key order).  A dot pixel lands at
   its linear address like the unchecked Mat::at (past the left/right edge it wraps into the
   neighbouring row); writes that would leave the canvas are dropped.
   h_random_idx (may be NULL): the n_key chosen match indices. */
erp_status erp_epipolar_draw_dev(erp_ctx* ctx, const erp_point2f* h_key_left,
                                 const erp_point2f* h_key_right, int32_t m, int32_t im_width,
                                 int32_t im_height, int32_t out_width, int32_t out_height,
                                 int32_t n_key, uint32_t seed, uint64_t offset, const double E[9],
                                 uint8_t* d_out, int32_t* h_random_idx, void* stream);
/* epipolar_tool's constructor choice (src/epipolar_tool.cpp:13-16), host only: the first n of
   std::random_shuffle(iota(m)) on the glibc rand() stream at (seed, offset) into h_idx (n <= m;
   the shuffle consumes m - 1 rand() calls).  The same indices erp_epipolar_draw_dev draws. */
erp_status erp_random_shuffle_prefix(uint32_t seed, uint64_t offset, int32_t m, int32_t n,
                                     int32_t* h_idx);
/* feature_matcher::draw_match (src/feature_matcher.cpp:61-86): d_out (W x H CV_8UC3) = the
   grey images of d_left / d_right (cvtColor CV_RGB2GRAY, as the reference calls it on its BGR
   images) in channels 0 / 1, 0 in channel 2, with a line of thickness 5 from key_left[i] to
   key_right[i] (device keypoints, rounded like cv::Point(Point2f)) in the colour
   HSV(i 180 / m, 180, 150) -> BGR, later matches on top.  Lines are the pixels within 2.5 of
   the segment (cv::line's thickness-5 rasteriser is not restated: parity with OpenCV is
   unpinned).  m <= 65535; the three image pointers are 4-byte aligned. */
erp_status erp_draw_match_dev(erp_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                              int32_t W, int32_t H, const erp_point2f* d_key_left,
                              const erp_point2f* d_key_right, int32_t m, uint8_t* d_out,
                              void* stream);

/* host 3x3 geometry (row-major doubles) */
void erp_eular2rot(const double theta[3], double R[9]);         /* erp_rotation.cpp:14-40 */
void erp_rot2eular(const double R[9], double e[3]);             /* erp_rotation.cpp:43-63 */
void erp_rot_from_vec(const double v1[3], const double v2[3], double R[9]); /* automatic.cpp:50-64 */
int32_t erp_inv3(const double m[9], double out[9]);            /* cv::Mat::inv() on 3x3 */
/* the two matrices rotate_pixel applies in rectify's rotate_image calls */
erp_status erp_rectify_matrices(const double rot_vec[3], const double t_vec[3], double m_left[9],
                                double m_right[9]);
/* host records -> the matrices of erp_rectify_results_dev (which goes through this): per record
   R, T widened to double, then erp_rectify_matrices into m_left / m_right [n][9]; ok[p] = 0
   (matrices unspecified) where status != ERP_OK or the pose is rejected, else 1 */
erp_status erp_rectify_matrices_results(const erp_pair_result* h_results, int32_t n,
                                        double* m_left, double* m_right, int32_t* ok);

#ifdef __cplusplus
}
#endif
#endif /* ERP_MATCH_H */

// erp_stage.hpp -- what every stage behind find does per pair (private; polish.hip, pose.hip,
// guided.hip, winner.hip): the limits, the prologue that decides whether a pair runs, the
// "record source" (a solved 9-vector per pair with an optional status), the copy of the result
// record with patched words, and the shared pieces of a "status and zeros" output.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/erp_match.h"

namespace erp {

constexpr int kStageMaxM = 65535;    // a pair's matches, as find: the polish's bitmaps are sized by it
constexpr int kPolishMaxRounds = 8;  // erp_polish_dev's limit (and find_posed's, which runs it)

// Each pair's solved 9-vector at e + p * e_stride (bytes) and, where status is not null, the
// int32 status of the record it lies in at status + p * status_stride: the e / src_status fields
// of erp_pose_inputs and erp_guided_inputs, or a field pair of a record array.
struct RecordSource {
    const void* e;
    int64_t e_stride;
    const void* status;
    int64_t status_stride;

    __device__ __forceinline__ const double* e_of(int p) const {
        return (const double*)((const char*)e + (size_t)p * e_stride);
    }
    __device__ __forceinline__ int32_t status_of(int p) const {  // ERP_OK without a status
        return status ? *(const int32_t*)((const char*)status + (size_t)p * status_stride)
                      : (int32_t)ERP_OK;
    }
};
template <class In>  // erp_pose_inputs, erp_guided_inputs
__host__ __device__ inline RecordSource source_of(const In& in) {
    return RecordSource{in.e, in.e_stride, in.src_status, in.src_status_stride};
}

// the host's argument rule for a source: e is required and 8-byte aligned at every pair, the
// status 4-byte aligned, no negative stride
inline bool source_ok(const RecordSource& s) {
    return s.e && s.e_stride >= 0 && (s.e_stride & 7) == 0 && ((uintptr_t)s.e & 7) == 0 &&
           (!s.status || (s.status_stride >= 0 && (s.status_stride & 3) == 0 &&
                          ((uintptr_t)s.status & 3) == 0));
}

// a pair's match count: the result record's M, never outside [0, key_stride]
__device__ __forceinline__ int64_t stage_match_count(const erp_pair_result* res, int64_t key_stride) {
    const int64_t m = res->M;
    return m < 0 ? 0 : (m > key_stride ? key_stride : m);
}

// Whether a pair runs: ERP_OK, or the status its outputs carry instead -- the result record's
// first, then ERP_INVALID_ARG for more than kStageMaxM matches, then the source's
// (RecordSource::status_of, or the winner record's).  Every input is the same for the whole
// block, so a branch on the answer is block-uniform.
__device__ __forceinline__ int32_t stage_gate(int32_t result_status, int64_t M,
                                              int32_t source_status) {
    if (result_status != ERP_OK) return result_status;
    if (M > kStageMaxM) return ERP_INVALID_ARG;
    return source_status;
}

// an output record of zeros that carries `status`
template <class T>
__device__ __forceinline__ T stage_record(int32_t status) {
    T o;
    memset(&o, 0, sizeof(o));
    o.status = status;
    return o;
}

// p[0, n) = 0 by a block of THREADS threads
template <int THREADS, class T>
__device__ __forceinline__ void stage_zero(T* p, int64_t n) {
    for (int64_t i = threadIdx.x; i < n; i += THREADS) p[i] = T(0);
}

// dst = src (dst may be src) moved as eight 64-bit words, so that every byte of the record is
// copied; patch(w) replaces the words of the fields to change in between
static_assert(sizeof(erp_pair_result) == 64 && offsetof(erp_pair_result, R) == 0 &&
                  offsetof(erp_pair_result, T) == 12 && offsetof(erp_pair_result, M) == 28,
              "R, T are words 0..2 and M the high half of word 3");
template <class Patch>
__device__ __forceinline__ void copy_result(erp_pair_result* dst, const erp_pair_result* src,
                                            Patch patch) {
    uint64_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = ((const uint64_t*)src)[k];
    patch(w);
#pragma unroll
    for (int k = 0; k < 8; k++) ((uint64_t*)dst)[k] = w[k];
}

}  // namespace erp

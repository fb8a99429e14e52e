// erp_host_stage.hpp -- the device side of the one-pair host entry points behind find
// (erp_eight_point_find_polished, erp_eight_point_find_posed, erp_match_guided,
// erp_eight_point_find_support): a bump layout and the four layouts built on it, all in the context's one kSlotHostStage.  Host only, plain
// C++17, no HIP types: a stand-alone g++ program checks it (tests/cpp/host_stage_check.cpp).
// Precondition: the slot's base address is at least 16-byte aligned (hipMalloc gives 256), so an
// offset's alignment is the address's.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/erp_match.h"

namespace erp {

struct StageLayout {
    size_t end = 0;
    // the offset of a part of `bytes` bytes aligned to `align`, behind the parts so far
    size_t add(size_t bytes, size_t align) {
        const size_t off = (end + align - 1) / align * align;
        end = off + bytes;
        return off;
    }
    // what to allocate: the parts and the 8 spare bytes these slots always had
    size_t total() const { return end + 8; }
};

// Each layout: the byte offset of every part, and bytes = the slot's size.
struct PolishedStage {
    size_t hyps, polish, wh, mask, bytes;
    PolishedStage(int32_t m, int32_t iters) {
        StageLayout l;
        hyps = l.add((size_t)iters * sizeof(erp_hypothesis), 8);
        polish = l.add(sizeof(erp_polish_result), 8);
        wh = l.add(2 * sizeof(int32_t), 4);
        mask = l.add((size_t)m, 1);
        bytes = l.total();
    }
};

struct PosedStage {
    size_t result, winner, polish, pose, wh, depth, mask, front, bytes;
    explicit PosedStage(int32_t m) {
        StageLayout l;
        result = l.add(sizeof(erp_pair_result), 8);
        winner = l.add(sizeof(erp_winner), 8);
        polish = l.add(sizeof(erp_polish_result), 8);
        pose = l.add(sizeof(erp_pose), 8);
        wh = l.add(2 * sizeof(int32_t), 4);
        depth = l.add((size_t)m * 2 * sizeof(double), 8);
        mask = l.add((size_t)m, 1);
        front = l.add((size_t)m, 1);
        bytes = l.total();
    }
};

struct GuidedStage {
    size_t e, off, desc1, desc2, matches, kp1, kp2, wh, count, bytes;
    GuidedStage(int32_t n1, int32_t n2) {
        constexpr size_t kRow = 64 * sizeof(float);  // a descriptor row; the kernels read float4s
        StageLayout l;
        e = l.add(9 * sizeof(double), 8);
        off = l.add(4 * sizeof(int64_t), 8);  // off_l[2], off_r[2]
        desc1 = l.add((size_t)n1 * kRow, 16);
        desc2 = l.add((size_t)n2 * kRow, 16);
        matches = l.add((size_t)n1 * sizeof(erp_dmatch), 4);
        kp1 = l.add((size_t)n1 * sizeof(erp_point2f), 8);
        kp2 = l.add((size_t)n2 * sizeof(erp_point2f), 8);
        wh = l.add(2 * sizeof(int32_t), 4);
        count = l.add(sizeof(int32_t), 4);
        bytes = l.total();
    }
};

struct SupportStage {
    size_t result, support, winner, support_result, counts, bytes;
    explicit SupportStage(int32_t iters) {
        StageLayout l;
        result = l.add(sizeof(erp_pair_result), 8);
        support = l.add(sizeof(erp_support), 4);
        winner = l.add(sizeof(erp_winner), 8);
        support_result = l.add(sizeof(erp_pair_result), 8);
        counts = l.add((size_t)iters * sizeof(int32_t), 4);
        bytes = l.total();
    }
};

}  // namespace erp

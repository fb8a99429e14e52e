// erp/rand_stream.hpp -- the glibc rand() stream that continues from one find to the next, as
// the reference's process-global rand() does (include/erp_match.h "rand stream" has the rules:
// which calls consume, how much, and in which order).
//
//   erp::eight_point ep;
//   ep.use_stream(&erp::rand_stream::process());   // the reference's semantics
#pragma once

#include <stdint.h>

#include "../erp_match.h"
#include "types.hpp"

namespace erp {

class rand_stream {
public:
    // an own stream: seeded with `seed`, `offset` draws consumed (host only until a GPU call
    // uses it)
    explicit rand_stream(uint32_t seed = 1, uint64_t offset = 0);
    ~rand_stream();
    rand_stream(const rand_stream&) = delete;
    rand_stream& operator=(const rand_stream&) = delete;

    // the process-wide stream of a device, at (1, 0) in a fresh process: glibc's global state
    static rand_stream& process(int device = 0);

    void get(uint32_t& seed, uint64_t& draws) const;  // waits for the last device update
    uint64_t draws() const;
    void set(uint32_t seed, uint64_t offset);
    void advance(uint64_t n);  // rand() calls made elsewhere (e.g. by FLANN)

    erp_rand_stream* handle() const { return s_; }

private:
    struct process_tag {};
    rand_stream(process_tag, int device);
    erp_rand_stream* s_ = nullptr;
    bool owned_ = true;
};

}  // namespace erp

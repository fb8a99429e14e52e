// Stand-alone host check of SupportStage in erp_match_eightpoint_test_amd/csrc/erp_host_stage.hpp
// (g++ -std=c++17, only that header), the device-side layout of erp_eight_point_find_support: for
// each iteration count every part lies inside the slot, no two parts overlap and every part is
// aligned to its element type (the records that hold doubles 8, int32 records and counts 4).  The
// part sizes are written out here on their own.  It then fills every part of a buffer of the
// slot's size with its own byte and reads all of them back, so that a sanitized build sees each
// byte the entry point's copies touch.  Prints one JSON line per shape; exit status 1 on a
// violated property.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../erp_match_eightpoint_test_amd/csrc/erp_host_stage.hpp"

namespace {

struct Part {
    const char* name;
    size_t off, bytes, align;
};

int fails = 0;

void check(const std::string& what, size_t total, const std::vector<Part>& parts) {
    for (size_t i = 0; i < parts.size(); i++) {
        const Part& a = parts[i];
        auto bad = [&](const std::string& why) {
            fprintf(stderr, "%s %s: %s (off %zu, %zu B, total %zu B)\n", what.c_str(), a.name,
                    why.c_str(), a.off, a.bytes, total);
            fails++;
        };
        if (a.off + a.bytes > total) bad("past the slot's end");
        if (a.off % a.align) bad("misaligned");
        for (size_t j = i + 1; j < parts.size(); j++) {
            const Part& b = parts[j];
            if (a.bytes && b.bytes && a.off < b.off + b.bytes && b.off < a.off + a.bytes)
                bad(std::string("overlaps ") + b.name);
        }
    }
    // every part written with its own byte, then read back: no part's bytes were another's
    std::vector<unsigned char> slot(total, 0xEE);
    for (size_t i = 0; i < parts.size(); i++)
        if (parts[i].off + parts[i].bytes <= total)
            memset(slot.data() + parts[i].off, (int)(i + 1), parts[i].bytes);
    for (size_t i = 0; i < parts.size(); i++)
        for (size_t k = 0; k < parts[i].bytes && parts[i].off + k < total; k++)
            if (slot[parts[i].off + k] != (unsigned char)(i + 1)) {
                fprintf(stderr, "%s %s: byte %zu overwritten\n", what.c_str(), parts[i].name, k);
                fails++;
                break;
            }
    printf("{\"entry\": \"%s\", \"bytes\": %zu", what.c_str(), total);
    for (const Part& p : parts) printf(", \"%s\": %zu", p.name, p.off);
    printf("}\n");
}

}  // namespace

int main() {
    static_assert(sizeof(erp_support) == 32 && sizeof(erp_support_outputs) == 4 * sizeof(void*),
                  "erp_support is eight int32, erp_support_outputs four pointers");
    for (int iters : {1, 31, 80, 10000, 100000}) {
        const erp::SupportStage s(iters);
        check("support " + std::to_string(iters), s.bytes,
              {{"result", s.result, 64, 8}, {"support", s.support, 32, 4},
               {"winner", s.winner, 88, 8}, {"support_result", s.support_result, 64, 8},
               {"counts", s.counts, (size_t)iters * 4, 4}});
    }
    return fails ? 1 : 0;
}

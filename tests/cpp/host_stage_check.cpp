// Stand-alone host check of erp_match_eightpoint_test_amd/csrc/erp_host_stage.hpp (g++
// -std=c++17, only that header): for each shape of the three one-pair entry points, every part
// lies inside the slot, no two parts overlap and every part is aligned to its element type
// (descriptor rows 16 bytes; doubles, int64 and the records that hold doubles 8; int32 and
// float 4).  The part sizes are written out here on their own.  Prints one JSON line per shape
// with the total and the offsets, which tests/test_host_stage_host.py compares with the
// offset chains the entry points computed by hand before.  Exit status 1 on a violated property.
#include <stdio.h>

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
    printf("{\"entry\": \"%s\", \"bytes\": %zu", what.c_str(), total);
    for (const Part& p : parts) printf(", \"%s\": %zu", p.name, p.off);
    printf("}\n");
}

}  // namespace

int main() {
    const int ms[] = {0, 1, 7, 64, 65535};
    for (int m : ms) {
        const size_t M = (size_t)m;
        for (int iters : {1, 80}) {
            const erp::PolishedStage s(m, iters);
            check("polished " + std::to_string(m) + " " + std::to_string(iters), s.bytes,
                  {{"hyps", s.hyps, (size_t)iters * 120, 8}, {"polish", s.polish, 120, 8},
                   {"wh", s.wh, 8, 4}, {"mask", s.mask, M, 1}});
        }
        const erp::PosedStage s(m);
        check("posed " + std::to_string(m), s.bytes,
              {{"result", s.result, 64, 8}, {"winner", s.winner, 88, 8}, {"polish", s.polish, 120, 8},
               {"pose", s.pose, 160, 8}, {"wh", s.wh, 8, 4}, {"depth", s.depth, M * 16, 8},
               {"mask", s.mask, M, 1}, {"front", s.front, M, 1}});
    }
    const int ns[][2] = {{0, 0}, {1, 2}, {33, 7}, {65535, 3}};
    for (const auto& n : ns) {
        const size_t n1 = (size_t)n[0], n2 = (size_t)n[1];
        const erp::GuidedStage s(n[0], n[1]);
        check("guided " + std::to_string(n[0]) + " " + std::to_string(n[1]), s.bytes,
              {{"e", s.e, 72, 8}, {"off", s.off, 32, 8}, {"desc1", s.desc1, n1 * 256, 16},
               {"desc2", s.desc2, n2 * 256, 16}, {"matches", s.matches, n1 * 16, 4},
               {"kp1", s.kp1, n1 * 8, 4}, {"kp2", s.kp2, n2 * 8, 4}, {"wh", s.wh, 8, 4},
               {"count", s.count, 4, 4}});
    }
    return fails ? 1 : 0;
}

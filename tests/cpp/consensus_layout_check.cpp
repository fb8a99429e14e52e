// Stand-alone host check of erp_match_eightpoint_test_amd/csrc/erp_consensus_ws.hpp (g++
// -std=c++17, nothing else included from the project): for each shape, every part lies inside
// its buffer, no two parts of a buffer overlap (sortbuf's two roles are the one declared alias)
// and every part meets its alignment.  Prints one JSON line per shape with the buffer sizes and
// part offsets, which tests/test_consensus_layout_host.py compares with the formulas it writes
// out on its own.  Exit status 1 on the first violated property.
#include <stdio.h>

#include <string>
#include <vector>

#include "../../erp_match_eightpoint_test_amd/csrc/erp_consensus_ws.hpp"

namespace {

struct Named {
    const char* name;
    erp::WsPart part;
    size_t need_align;  // what the part's element type asks for
};

int fails = 0;

void check_buffer(const char* buf, size_t bytes, const std::vector<Named>& parts, int P, int iters) {
    for (size_t i = 0; i < parts.size(); i++) {
        const erp::WsPart& a = parts[i].part;
        auto bad = [&](const char* what) {
            fprintf(stderr, "(%d, %d) %s.%s: %s (off %zu, %zu x %zu B, buffer %zu B)\n", P, iters, buf,
                    parts[i].name, what, a.off, a.count, a.elem, bytes);
            fails++;
        };
        if (a.end() > bytes) bad("past the buffer's end");
        if (a.off % parts[i].need_align || a.align != parts[i].need_align) bad("misaligned");
        for (size_t j = i + 1; j < parts.size(); j++) {
            const erp::WsPart& b = parts[j].part;
            if (a.off < b.end() && b.off < a.end()) bad((std::string("overlaps ") + parts[j].name).c_str());
        }
    }
}

void print_parts(const char* buf, size_t bytes, const std::vector<Named>& parts, bool last = false) {
    printf("\"%s\": {\"bytes\": %zu", buf, bytes);
    for (const Named& n : parts) printf(", \"%s\": [%zu, %zu]", n.name, n.part.off, n.part.count);
    printf(last ? "}" : "}, ");
}

void run(int P, int iters) {
    const erp::ConsensusLayout l = erp::consensus_layout(P, iters);
    const auto& r = l.lipref;
    const std::vector<Named> counts = {{"nsurv", l.counts.nsurv, 4}, {"nbin", l.counts.nbin, 4},
                                       {"uoff", l.counts.uoff, 4}, {"n2", l.counts.n2, 4},
                                       {"nfb", l.counts.nfb, 4}};
    const std::vector<Named> edges = {{"first", l.edges.first, 4}, {"zoom", l.edges.zoom, 4},
                                      {"zgrid", l.edges.zgrid, 4}};
    const std::vector<Named> lipref = {{"ref", r.ref, 16}, {"U", r.U, 8}, {"cnt", r.cnt, 4},
                                       {"r2cnt", r.r2cnt, 4}, {"r2list", r.r2list, 4},
                                       {"gref", r.gref, 16}, {"gsel", r.gsel, 4}, {"gcnt", r.gcnt, 4},
                                       {"goff", r.goff, 4}, {"nflat", r.nflat, 4},
                                       {"hcand", r.hcand, 16}};
    // sortbuf: the float scratch and list2 are the declared alias -- checked one role at a time
    const std::vector<Named> score = {{"score", l.sortbuf.score, 4}};
    const std::vector<Named> list2 = {{"list2", l.sortbuf.list2, 4}};
    const std::vector<Named> hlite = {{"hl", l.hlite.hl, 4}, {"wsum", l.hlite.wsum, 4}};
    const std::vector<Named> rtab = {{"recip", l.rtab.recip, 8}, {"magic", l.rtab.magic, 8},
                                     {"bad", l.rtab.bad, 4}};
    check_buffer("nsurv", l.counts.bytes, counts, P, iters);
    check_buffer("edges", l.edges.bytes, edges, P, iters);
    check_buffer("lipref", r.bytes, lipref, P, iters);
    check_buffer("sortbuf", l.sortbuf.bytes, score, P, iters);
    check_buffer("sortbuf", l.sortbuf.bytes, list2, P, iters);
    check_buffer("hlite", l.hlite.bytes, hlite, P, iters);
    check_buffer("rtab", l.rtab.bytes, rtab, P, iters);
    // both of list2's strides fit a pair's share of sortbuf, and the snapshot's share of lipref
    // is the contiguous head ref, U, cnt
    const size_t S = 2 * (size_t)iters;
    if (l.sortbuf.list2_bounds_stride != S || l.sortbuf.list2_refine_stride != l.sortbuf.len ||
        S > l.sortbuf.len || l.sortbuf.list2.count != (size_t)P * l.sortbuf.len ||
        r.ref.off != 0 || r.U.off != r.ref.end() || r.cnt.off != r.U.end() ||
        r.snap_bytes != r.cnt.end() || r.ref.count != (size_t)P * r.cap ||
        r.gref.count != (size_t)P * r.gcap * 2) {
        fprintf(stderr, "(%d, %d): list2 strides / snapshot head inconsistent\n", P, iters);
        fails++;
    }
    printf("{\"n_pairs\": %d, \"iters\": %d, \"lb\": %zu, \"ub\": %zu, \"bsel\": %zu, \"zsel\": %zu, "
           "\"surv\": %zu, \"cap\": %zu, \"gcap\": %zu, \"sortbuf_len\": %zu, \"snap\": %zu, ",
           P, iters, l.lb_bytes, l.ub_bytes, l.bsel_bytes, l.zsel_bytes, l.surv_bytes, r.cap, r.gcap,
           l.sortbuf.len, r.snap_bytes);
    print_parts("nsurv", l.counts.bytes, counts);
    print_parts("edges", l.edges.bytes, edges);
    print_parts("lipref", r.bytes, lipref);
    print_parts("sortbuf", l.sortbuf.bytes, {score[0], list2[0]});
    print_parts("hlite", l.hlite.bytes, hlite);
    print_parts("rtab", l.rtab.bytes, rtab, true);
    printf("}\n");
}

}  // namespace

int main() {
    const int shapes[][2] = {{1, 1}, {1, 80}, {3, 33}, {9, 1100}, {128, 10000}, {768, 10000}, {1, 100000}};
    for (const auto& s : shapes) run(s[0], s[1]);
    return fails ? 1 : 0;
}

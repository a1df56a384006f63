// Host-only harness for tests/test_conv_select_cpu.py: replays conv_select (csrc/conv_select.h) on cases read from stdin.
// One case per line, whitespace-separated integers: the ConvSelIn fields, then the plan options, in the order of the two name lists `--fields` prints
// (a third line names the result columns).  One output line per case: the ConvSel fields as integers, then the label tag.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "conv_select.h"
using namespace td;

static const char* const kIn[] = {"N", "h", "w", "cout", "cout_pad", "kgroups", "nseg",
                                  "s0_C", "s0_taps", "s0_xform", "s0_resample", "s0_Hs", "s0_Ws", "s1_C", "s1_taps", "s1_xform", "s1_resample", "s1_Hs", "s1_Ws",
                                  "s2_C", "s2_taps", "s2_xform", "s2_resample", "s2_Hs", "s2_Ws",
                                  "chunk", "dt", "bf16", "sb_n3", "out_f32", "epi", "has_res", "clip_pos", "n_cus", "op_index"};
static const char* const kOut[] = {"kernel", "narrow", "bn", "glds_variant", "sb_mt", "sb_nt", "tiles_x", "tiles_y", "img_groups", "n_ntiles", "ksplit", "persist",
                                   "sb_order", "reverse", "dma1x1", "out_parts", "wcopy"};

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--fields") {
        for (const char* n : kIn) printf("%s ", n);
        printf("\n");
        PlanOptions o{};
        o.for_each([](const char* n, int64_t&) { printf("%s ", n); });
        printf("\n");
        for (const char* n : kOut) printf("%s ", n);
        printf("\n");
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        ConvSelIn in;
        PlanOptions o{};
        is >> in.N >> in.h >> in.w >> in.cout >> in.cout_pad >> in.kgroups >> in.nseg;
        for (ConvSelSeg& s : in.seg) is >> s.C >> s.taps >> s.xform >> s.resample >> s.Hs >> s.Ws;
        is >> in.chunk >> in.dt >> in.bf16 >> in.sb_n3 >> in.out_f32 >> in.epi >> in.has_res >> in.clip_pos >> in.n_cus >> in.op_index;
        o.for_each([&](const char*, int64_t& v) { is >> v; });
        if (!is || in.nseg < 0 || in.nseg > 3) { fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        const ConvSel s = conv_select(in, o);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\n", (int)s.kernel, (int)s.narrow, s.bn, s.glds_variant, s.sb_mt, s.sb_nt, s.tiles_x, s.tiles_y, s.img_groups,
               s.n_ntiles, s.ksplit, s.persist, s.sb_order, s.reverse, s.dma1x1, s.out_parts, (int)s.wcopy, conv_sel_tag(s).c_str());
    }
    return 0;
}

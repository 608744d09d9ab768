// The library's own plan of a batch call (csrc/batch_plan.cpp, plan_batch) for the groups calls of tests/history_cases.py:
//   history_plan_check n  nwin Hc Wc  [nwin Hc Wc ...]
// prints "total <stage-plane bytes> tab <descriptor-table bytes> subs <sub-batches> vec <labeller word width>", then one line per
// group: "group g sub <k> pitch <elements> goff <byte offset> P <Hc * Wc>".  Dense host BGR groups with records, as the tests pass
// them.  Plain C++: no device, nothing loaded into Python (tests/test_history_independence_cpu.py builds and runs it).
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "batch_plan.h"

int main(int argc, char **argv)
{
    if (argc < 5 || (argc - 2) % 3) { fprintf(stderr, "usage: history_plan_check n nwin Hc Wc ...\n"); return 2; }
    const int n = atoi(argv[1]), G = (argc - 2) / 3;
    std::vector<swk_input> in(G);
    std::vector<swk_output> out(G);
    static uint8_t frames[16];
    static swk_segment segs[1];
    static int32_t nseg[1];
    for (int g = 0; g < G; ++g) {
        swk_input i{};
        i.frames = frames;          // never read: the plan is integer arithmetic on the descriptions
        i.mem = SWK_MEM_HOST;
        i.channels = 3;
        i.nwin = atoi(argv[2 + 3 * g]); i.n = n; i.Hc = atoi(argv[3 + 3 * g]); i.Wc = atoi(argv[4 + 3 * g]);
        i.x0 = i.y0 = 0;
        i.row_stride = (int64_t)i.Wc * 3;
        i.frame_stride = (int64_t)i.Hc * i.row_stride;
        in[g] = i;
        swk_output o{};
        o.mem = SWK_MEM_HOST;
        o.seg_cap = 255; o.segs = segs; o.nseg = nseg;
        out[g] = o;
    }
    swk::BatchPlan plan;
    const char *why = "";
    const int rc = swk::plan_batch(in.data(), G, out.data(), &plan, &why);
    if (rc) { fprintf(stderr, "refused: %s\n", why); return 1; }
    printf("total %zu tab %zu subs %zu vec %d\n", plan.total, plan.tab_bytes, plan.subs.size(), plan.vec);
    for (int g = 0; g < G; ++g)
        printf("group %d sub %d pitch %d goff %lld P %d\n", g, plan.grp[g].sub, plan.grp[g].pitch, (long long)plan.grp[g].goff,
               in[g].Hc * in[g].Wc);
    return 0;
}

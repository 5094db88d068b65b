// Prints the render plan (csrc/path_plan.h) of every case read from stdin, one line each; includes
// nothing but the HIP-free headers.  tests/test_plan_host.py feeds it tests/golden/path_plan_cases.json.
//   case:  N M spp max_depth cont subset n_tris bvh_dev_bytes grid0 grid1 grid2 block [option=value ...]
//   plan:  key=value ..., a launch as L<k>=kind,grid,list,order_mode,prio,mix,contrib_lanes
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "path_plan.h"

using namespace akr;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        PathPlanIn in;
        Options o;
        int cont = 0, subset = 0;
        ss >> in.N >> in.M >> in.spp >> in.max_depth >> cont >> subset >> in.n_tris >> in.bvh_dev_bytes >> in.grid[0] >>
            in.grid[1] >> in.grid[2] >> in.block;
        if (!ss) {
            std::printf("error: short case line\n");
            return 2;
        }
        in.cont = cont != 0;
        in.subset = subset != 0;
        std::string kv;
        while (ss >> kv) {
            const size_t eq = kv.find('=');
            const std::string why = eq == std::string::npos ? "no value for " + kv
                                                            : set_option(o, kv.substr(0, eq).c_str(), std::stoll(kv.substr(eq + 1)));
            if (!why.empty()) {
                std::printf("error: %s\n", why.c_str());
                return 2;
            }
        }
        const PathPlan p = plan_path(in, o);
        std::printf("ppl1000=%lld order_min_spp=%d pilot=%d path_pilot=%d want_steps=%d pilot_rays=%lld gated=%d n_launch=%d "
                    "last_form=%d gate_forms=%d,%d last_ordered=%d",
                    (long long)p.ppl1000, p.order_min_spp, (int)p.pilot, (int)p.path_pilot, (int)p.want_steps,
                    (long long)p.pilot_rays, (int)p.gated, p.n_launch, p.last_form, p.gate_forms[0], p.gate_forms[1],
                    p.last_ordered);
        for (int k = 0; k < p.n_launch; k++) {
            const PathLaunch &l = p.launch[k];
            std::printf(" L%d=%d,%u,%d,%u,%u,%u,%llu", k, l.kind, l.grid, l.list, l.order_mode, l.prio, l.mix,
                        (unsigned long long)l.contrib_lanes);
        }
        std::printf("\n");
    }
    return 0;
}

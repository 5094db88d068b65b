// env_forms_check.cpp — option "env_forms" (csrc/options.h) and what it does to the render plan
// (csrc/path_plan.h env_plain_only), the host half of k_path_defer's and k_path_spec's environment builds
// (DESIGN.md §0.8).  Includes nothing but the HIP-free headers.
//   env_forms_check          the option's checks: one line per check that fails, "ok <checks>" at the end; the
//                            exit status is the number of failures
//   env_forms_check plans    the plan of every case read from stdin, as a render under an environment with
//                            env_path 1 and env_forms 1 builds its PathPlanIn; path_plan_check.cpp's formats
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "path_plan.h"

using namespace akr;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            g_failed++;                                              \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
        }                                                            \
    } while (0)

static void set(Options &o, const char *key, int64_t v) {
    const std::string why = set_option(o, key, v);
    g_checks++;
    if (!why.empty()) {
        g_failed++;
        std::printf("FAILED: set_option(%s, %lld): %s\n", key, (long long)v, why.c_str());
    }
}

static int plans() {
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
        if (!o.env_path || !o.env_forms) {
            std::printf("error: a case line without env_path=1 env_forms=1\n");
            return 2;
        }
        in.plain_only = env_plain_only(true, o);  // an environment is set
        const PathPlan p = plan_path(in, o);
        std::printf("plain_only=%d ppl1000=%lld order_min_spp=%d pilot=%d path_pilot=%d want_steps=%d pilot_rays=%lld gated=%d "
                    "n_launch=%d last_form=%d gate_forms=%d,%d last_ordered=%d",
                    (int)in.plain_only, (long long)p.ppl1000, p.order_min_spp, (int)p.pilot, (int)p.path_pilot, (int)p.want_steps,
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

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "plans") == 0) return plans();
    {  // the option: 0 / 1, default 0, anything else refused with its message and nothing stored
        Options o;
        CHECK(!o.env_forms);
        set(o, "env_forms", 1);
        CHECK(o.env_forms);
        CHECK(set_option(o, "env_forms", 2) == "env_forms must be in [0, 1]");
        CHECK(o.env_forms);
        CHECK(set_option(o, "env_forms", -1) == "env_forms must be in [0, 1]");
        CHECK(o.env_forms);
        set(o, "env_forms", 0);
        CHECK(!o.env_forms);
        CHECK(set_option(o, "env_forms", 2) == "env_forms must be in [0, 1]");
        CHECK(set_option(o, "env_forms", -1) == "env_forms must be in [0, 1]");
        CHECK(set_option(o, "env_forms", INT64_MAX) == "env_forms must be in [0, 1]");
        CHECK(!o.env_forms);
        // it is a key of its own: env_path and the options beside it keep their values, and env_path its meaning
        Options d;
        set(o, "env_forms", 1);
        CHECK(!o.env_path && o.path_kernel == d.path_kernel && o.path_defer == d.path_defer && o.path_spec == d.path_spec &&
              o.mis == d.mis && o.film_variance == d.film_variance);
        set(o, "env_path", 1);
        CHECK(o.env_path && o.env_forms);
        CHECK(set_option(o, "env_path", 2) == "env_path must be in [0, 1]");
        set(o, "env_path", 0);
        CHECK(!o.env_path && o.env_forms);
    }
    {  // matched before the table: no row, and the table is the one it was (tests/golden/options.json: 47 rows)
        CHECK(find_option("env_forms") == nullptr);
        CHECK(find_option("env_path") == nullptr);
        CHECK(sizeof(kOptionTable) / sizeof(kOptionTable[0]) == 47);
        bool named = false;
        for (const OptionRow &r : kOptionTable) named = named || std::strstr(r.name, "env_") != nullptr;
        CHECK(!named);
        CHECK(std::strcmp(kOptionTable[0].name, "stats") == 0 && std::strcmp(kOptionTable[46].name, "rays_per_lane") == 0);
        // every row's default is untouched by setting the switch
        Options o, d;
        set(o, "env_forms", 1);
        for (const OptionRow &r : kOptionTable) CHECK(get_option(o, r) == get_option(d, r));
    }
    {  // what the render derives from it
        Options o;
        CHECK(!env_plain_only(false, o));  // no environment: nothing to limit
        CHECK(env_plain_only(true, o));    // env_path alone: k_path's build only
        set(o, "env_forms", 1);
        CHECK(!env_plain_only(true, o));
        CHECK(!env_plain_only(false, o));
        // forced forms come back under an environment, and go when the switch does
        PathPlanIn in;
        in.N = in.M = 1920ull * 1080ull;
        in.spp = 16;
        in.max_depth = 5;
        in.n_tris = 10000000;
        in.bvh_dev_bytes = 1500ull << 20;
        in.grid[PATH_PLAIN] = in.grid[PATH_DEFER] = in.grid[PATH_SPEC] = 1024;
        set(o, "path_defer", 1);
        in.plain_only = env_plain_only(true, o);
        PathPlan p = plan_path(in, o);
        CHECK(p.launch[0].kind == PATH_DEFER && p.last_form == AKR_FORM_PATH_DEFER && p.launch[0].contrib_lanes == 1024ull * 256);
        set(o, "path_defer", 0);
        set(o, "path_spec", 1);
        p = plan_path(in, o);
        CHECK(p.launch[0].kind == PATH_SPEC && p.last_form == AKR_FORM_PATH_SPEC && p.launch[0].contrib_lanes == 0);
        in.max_depth = 9;  // k_path_defer holds eight shadow slots: above max_depth 8 the forced form is k_path
        set(o, "path_spec", 0);
        set(o, "path_defer", 1);
        p = plan_path(in, o);
        CHECK(p.launch[0].kind == PATH_PLAIN && p.last_form == AKR_FORM_PATH);
        in.max_depth = 5;
        set(o, "env_forms", 0);
        in.plain_only = env_plain_only(true, o);
        p = plan_path(in, o);
        CHECK(p.launch[0].kind == PATH_PLAIN && p.last_form == AKR_FORM_PATH && !p.gated && p.n_launch == 1);
    }
    std::printf("ok %d\n", g_checks - g_failed);
    return g_failed;
}

// env_path_check.cpp — option "env_path" (csrc/options.h) and PathPlanIn::plain_only (csrc/path_plan.h), the
// host half of k_path's environment build.  Includes nothing but the HIP-free headers.
// Prints one line per check that fails and "ok <checks>" at the end; the exit status is the number of failures.
#include <cstdio>
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

// 1080p whole frame, 16 spp, depth 5, the grids of a 256-CU device
static PathPlanIn frame(uint64_t n_tris, uint64_t bvh_bytes) {
    PathPlanIn in;
    in.N = in.M = 1920ull * 1080ull;
    in.spp = 16;
    in.max_depth = 5;
    in.n_tris = n_tris;
    in.bvh_dev_bytes = bvh_bytes;
    in.grid[PATH_PLAIN] = in.grid[PATH_DEFER] = in.grid[PATH_SPEC] = 1024;
    in.block = 256;
    return in;
}

// with plain_only: one ungated k_path launch, whatever the other fields say
static void check_plain(const PathPlanIn &base, const Options &o, int want_list) {
    PathPlanIn in = base;
    in.plain_only = true;
    const PathPlan p = plan_path(in, o);
    CHECK(p.n_launch == 1);
    CHECK(!p.gated);
    CHECK(!p.want_steps);
    CHECK(p.launch[0].kind == PATH_PLAIN);
    CHECK(p.launch[0].contrib_lanes == 0);
    CHECK(p.launch[0].mix == 0);
    CHECK(p.launch[0].list == want_list);
    CHECK(p.last_form == AKR_FORM_PATH);
    CHECK(p.gate_forms[0] == AKR_FORM_NONE && p.gate_forms[1] == AKR_FORM_NONE);
    CHECK(p.launch[0].grid >= 1 && p.launch[0].grid <= in.grid[PATH_PLAIN]);
    // the fields the form does not touch are those of the same plan without the flag
    const PathPlan q = plan_path(base, o);
    CHECK(p.ppl1000 == q.ppl1000);
    CHECK(p.order_min_spp == q.order_min_spp);
}

int main() {
    {  // the option: 0 / 1, anything else refused and nothing stored; no row of the table
        Options o;
        CHECK(!o.env_path);
        CHECK(find_option("env_path") == nullptr);
        set(o, "env_path", 1);
        CHECK(o.env_path);
        CHECK(set_option(o, "env_path", 2) == "env_path must be in [0, 1]");
        CHECK(o.env_path);
        CHECK(set_option(o, "env_path", -1) == "env_path must be in [0, 1]");
        CHECK(o.env_path);
        set(o, "env_path", 0);
        CHECK(!o.env_path);
        CHECK(set_option(o, "env_path", -1) == "env_path must be in [0, 1]");
        CHECK(set_option(o, "env_path", 2) == "env_path must be in [0, 1]");
        CHECK(!o.env_path);
        // it leaves the options beside it alone
        Options d;
        CHECK(o.path_kernel == d.path_kernel && o.path_defer == d.path_defer && o.path_spec == d.path_spec && o.mis == d.mis);
    }
    const uint64_t big = 1500ull << 20, small = 1ull << 20;  // a tree past the cache share, and one inside it
    {  // a gated plan today: the default options on a large tree at a 4-way share's size
        Options o;
        PathPlanIn in = frame(10000000, big);
        in.N = in.M = in.N / 4;
        const PathPlan q = plan_path(in, o);
        CHECK(q.gated && q.n_launch == 2 && q.last_form == AKR_FORM_NONE);
        CHECK(q.launch[1].kind != PATH_PLAIN);
        check_plain(in, o, LIST_PILOT);
    }
    {  // k_path_defer forced
        Options o;
        set(o, "path_defer", 1);
        const PathPlanIn in = frame(10000000, big);
        const PathPlan q = plan_path(in, o);
        CHECK(!q.gated && q.launch[0].kind == PATH_DEFER && q.last_form == AKR_FORM_PATH_DEFER);
        CHECK(q.launch[0].contrib_lanes > 0);
        check_plain(in, o, LIST_PILOT);
    }
    {  // k_path_spec forced
        Options o;
        set(o, "path_spec", 1);
        const PathPlanIn in = frame(10000000, big);
        const PathPlan q = plan_path(in, o);
        CHECK(!q.gated && q.launch[0].kind == PATH_SPEC && q.last_form == AKR_FORM_PATH_SPEC);
        check_plain(in, o, LIST_PILOT);
    }
    {  // a cache-resident tree: the rule's tail form is k_path_defer at every size
        Options o;
        const PathPlanIn in = frame(36, small);
        const PathPlan q = plan_path(in, o);
        CHECK(q.gated && q.n_launch == 2 && q.launch[1].kind == PATH_DEFER && q.gate_forms[1] == AKR_FORM_PATH_DEFER);
        check_plain(in, o, LIST_PILOT);
    }
    {  // a subset pass (a masked continue) under forced k_path_defer: the list stays the subset's, linear
        Options o;
        set(o, "path_defer", 1);
        PathPlanIn in = frame(36, small);
        in.cont = in.subset = true;
        in.M = 5000;
        const PathPlan q = plan_path(in, o);
        CHECK(q.launch[0].kind == PATH_DEFER && q.launch[0].list == LIST_SUBSET && q.launch[0].order_mode == FETCH_SCRAMBLE);
        check_plain(in, o, LIST_SUBSET);
        in.plain_only = true;
        const PathPlan p = plan_path(in, o);
        CHECK(p.launch[0].order_mode == FETCH_LINEAR && !p.pilot && p.last_ordered == 0);
        CHECK(p.launch[0].grid == (5000 + 255) / 256);
    }
    {  // the knobs of k_path apply: path_grid_pct, path_prio, the pilot's kind, path_order 0
        Options o;
        set(o, "path_grid_pct", 50);
        set(o, "path_prio", 64);
        set(o, "path_order_pilot_spp", 2);
        PathPlanIn in = frame(10000000, big);
        in.plain_only = true;
        PathPlan p = plan_path(in, o);
        CHECK(p.launch[0].grid == 512 && p.launch[0].prio == 64 && p.pilot && p.path_pilot && p.last_ordered == 1);
        in.cont = true;  // a continue ranks by the camera-ray pilot
        p = plan_path(in, o);
        CHECK(p.pilot && !p.path_pilot && !p.want_steps);
        set(o, "path_order", 0);
        p = plan_path(in, o);
        CHECK(!p.pilot && p.launch[0].list == LIST_NONE && p.last_ordered == 0 && p.launch[0].kind == PATH_PLAIN);
        set(o, "path_order", 1);  // the pilot's order is k_path's alone: it still ranks here
        set(o, "path_defer", 1);
        p = plan_path(in, o);
        CHECK(p.pilot && p.launch[0].list == LIST_PILOT && p.launch[0].kind == PATH_PLAIN);
    }
    std::printf("ok %d\n", g_checks - g_failed);
    return g_failed;
}

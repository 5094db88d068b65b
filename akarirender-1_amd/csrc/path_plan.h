// path_plan.h — the render form rule of the persistent path kernels as a function of
// integers: which of k_path, k_path_defer and k_path_spec runs, whether a pilot ranks the pixels first,
// whether two gated candidates are launched, and each candidate's grid and fetch order.  Plain C++, no
// HIP header: capi.hip's render_path() carries the plan out, tests/cpp/path_plan_check.cpp exercises it.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/akr_hip.h"  // AKR_FORM_*
#include "akr_path_forms.h"
#include "options.h"

namespace akr {

struct PathPlanIn {
    uint64_t N = 0;            // the session's slots
    uint64_t M = 0;            // the slots this pass fetches (a subset pass: the list's length)
    int32_t spp = 0, max_depth = 0;
    bool cont = false;         // a continued render
    bool subset = false;       // a slot list is given (a masked continue)
    uint64_t n_tris = 0;
    uint64_t bvh_dev_bytes = 0;   // the uploaded wide nodes + leaf blob
    uint32_t grid[3] = {0, 0, 0}; // resident workgroups of each kernel form [kind], for the render's `tab`
    uint32_t block = 256;         // threads per workgroup of the path kernels
    // only PATH_PLAIN is taken for this render (an environment light under option env_path without option
    // env_forms): one ungated k_path launch whatever path_defer / path_spec and the cache rule
    // say; the pilot, the cost order, subset lists, path_grid_pct and path_prio apply as for k_path.  With
    // env_forms every form has an environment kernel and the flag stays false (env_plain_only)
    bool plain_only = false;
};

// PathPlanIn::plain_only of a persistent render: set under an environment unless option env_forms lifts it
// (render_path() is reached under an environment only with option env_path on)
inline bool env_plain_only(bool env_on, const Options &o) { return env_on && !o.env_forms; }

// which list a launch fetches its slots through
enum : int { LIST_NONE = 0, LIST_PILOT = 1, LIST_SUBSET = 2 };

struct PathLaunch {
    int kind = PATH_PLAIN;
    uint32_t grid = 0;
    int list = LIST_NONE;
    uint32_t order_mode = FETCH_LINEAR, prio = 0, mix = 0;
    uint64_t contrib_lanes = 0;  // k_path_defer: the lanes d_contrib must hold records for (else 0)
};

struct PathPlan {
    int64_t ppl1000 = 0;       // pixels per resident lane of k_path x 1000
    int order_min_spp = 0;     // the cost order's spp floor for this render
    bool pilot = false;        // a pilot ranks the slots ...
    bool path_pilot = false;   // ... by a counting k_path render (else by a camera ray's steps)
    bool want_steps = false;   // the camera-ray pilot also sums its steps (the rule's tail test)
    int64_t pilot_rays = -1;   // the rays that sum is over (-1: unused)
    bool gated = false;        // two candidates are launched; the device's gate word picks launch[gate]
    int n_launch = 1;
    PathLaunch launch[2];
    int32_t last_form = AKR_FORM_NONE;                          // AKR_FORM_NONE when gated: read from the gate
    int32_t gate_forms[2] = {AKR_FORM_NONE, AKR_FORM_NONE};     // gated only
    int32_t last_ordered = 0;
};

// The cost order's spp floor: a rank's share takes the order from fewer samples
inline int order_min_spp(const Options &o, uint64_t N) {
    return (int64_t)N <= o.path_order_share_pixels ? std::min(o.path_order_share_min_spp, o.path_order_min_spp)
                                                   : o.path_order_min_spp;
}

inline int32_t form_of(int kind) {
    return kind == PATH_SPEC ? AKR_FORM_PATH_SPEC : (kind == PATH_DEFER ? AKR_FORM_PATH_DEFER : AKR_FORM_PATH);
}

inline PathPlan plan_path(const PathPlanIn &in, const Options &o) {
    PathPlan pl;
    const uint64_t N = in.N, M = in.M;
    // pixels per resident lane of k_path (the occupancy query's grid)
    const uint64_t lanes = std::max<uint64_t>(1, (uint64_t)in.grid[PATH_PLAIN] * (uint64_t)o.path_grid_pct / 100) * in.block;
    const int64_t ppl1000 = (int64_t)((M * 1000 + lanes / 2) / lanes);
    pl.ppl1000 = ppl1000;
    pl.order_min_spp = order_min_spp(o, N);
    // plain_only: the form is given, as if path_defer 0 / path_spec 0 had forced k_path
    const int path_spec = in.plain_only ? 0 : o.path_spec, path_defer = in.plain_only ? 0 : o.path_defer;
    const bool forced = path_spec == 1 || path_defer != 2;
    // the pilot can rank pixels for every form (path_order 2), or for k_path only (1)
    pl.pilot = o.path_order != 0 && !in.subset && in.spp >= pl.order_min_spp && N >= 2 &&
               (o.path_order == 2 || (!forced || (path_spec != 1 && path_defer == 0)));
    // a continued render ranks by the camera-ray pilot: the path pilot renders into the film
    pl.path_pilot = pl.pilot && o.path_order_pilot_spp > 0 && !in.cont;
    // the rule: its size and scene tests, then the camera-ray pilot's mean steps
    const bool size_ok = ppl1000 <= o.path_tail_ppl10 * 100;
    const bool tris_ok = o.path_defer_min_tris == 0 || (int64_t)in.n_tris >= o.path_defer_min_tris;
    // the BVH's device bytes against the Infinity Cache share: a cache-resident
    // tree takes k_path_defer at any size, a larger one k_path_spec up to path_tail_ppl10
    const bool cache_resident = path_spec != 1 && in.max_depth <= 8 && in.bvh_dev_bytes <= (uint64_t)o.path_cache_mb << 20;
    const bool size_tail = path_spec == 2 ? (o.path_spec_pixels > 0 ? (int64_t)N <= o.path_spec_pixels : size_ok)
                                          : (o.path_defer_pixels > 0 ? (int64_t)N <= o.path_defer_pixels : size_ok);
    pl.want_steps = !forced && o.path_order == 2 && pl.pilot && !pl.path_pilot && tris_ok && (cache_resident || size_tail);
    if (pl.want_steps) pl.pilot_rays = (int64_t)((N + (1u << o.path_order_sub) - 1) >> o.path_order_sub);
    // The rule's tail test reads the pilot's step sum, which is on the device: both candidates are
    // launched, and each exits at once unless the gate word names it
    const int tail_kind = cache_resident ? PATH_DEFER
                                         : (path_spec == 2 ? PATH_SPEC : (in.max_depth <= 8 ? PATH_DEFER : PATH_PLAIN));
    pl.gated = pl.want_steps && tail_kind != PATH_PLAIN;
    int kind = PATH_PLAIN;
    if (path_spec == 1) kind = PATH_SPEC;
    else if (path_defer == 1 && in.max_depth <= 8) kind = PATH_DEFER;

    // one candidate's grid and fetch order
    auto configure = [&](int k) {
        PathLaunch x;
        x.kind = k;
        const uint64_t resident = (uint64_t)in.grid[k] * (uint64_t)o.path_grid_pct / 100;
        x.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(resident, (M + in.block - 1) / in.block));
        if (k == PATH_DEFER) {
            x.contrib_lanes = (uint64_t)x.grid * in.block;
            x.mix = o.path_mix ? 1u : 0u;
        }
        if (in.subset) {  // the active list in ascending order (k_path_defer keeps its scramble)
            x.list = LIST_SUBSET;
            x.order_mode = k == PATH_DEFER && o.path_mix ? FETCH_SCRAMBLE : FETCH_LINEAR;
            return x;
        }
        // path_order 1: the pilot's order is k_path's alone
        if (!pl.pilot || !(k == PATH_PLAIN || o.path_order == 2)) return x;
        x.list = LIST_PILOT;
        const bool small = ppl1000 <= 1500;  // at most 1.5 pixels per resident lane (8-way share)
        const bool pair = o.path_order_pair == 3 ||
                          (k != PATH_PLAIN && (o.path_order_pair == 1 || (o.path_order_pair == 2 && small)));
        x.order_mode = pair ? FETCH_PAIR : FETCH_LINEAR;
        // k_path_spec: every wave takes pixels from the whole cost order (FETCH_STRIDE), so
        // each has cheap pixels whose lanes turn helpers early (option path_spec_fetch)
        if (k == PATH_SPEC && o.path_spec_fetch >= 0 &&
            (o.path_spec_fetch_pixels > 0 ? (int64_t)N <= o.path_spec_fetch_pixels : small))
            x.order_mode = (uint32_t)o.path_spec_fetch;
        x.prio = (uint32_t)o.path_prio;
        return x;
    };
    if (pl.gated) {
        pl.n_launch = 2;
        pl.launch[0] = configure(PATH_PLAIN);
        pl.launch[1] = configure(tail_kind);
        pl.gate_forms[0] = form_of(PATH_PLAIN);
        pl.gate_forms[1] = form_of(tail_kind);
    } else {
        pl.launch[0] = configure(kind);
        pl.last_form = form_of(kind);
    }
    // after a gated launch this follows the plain candidate's order
    pl.last_ordered = pl.launch[0].list == LIST_PILOT ? 1 : 0;
    return pl;
}

}  // namespace akr

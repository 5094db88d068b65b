// options.h — every knob akr_hip_set_option sets: its field and default (with the measurements that chose
// it), and the table that maps an option name to its field, kind and bounds.  Plain C++, no HIP header.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

namespace akr {

struct Options {
    // In-band check that every slot of a render's film holds exactly spp samples (option "verify",
    // default on): device counter + mapped host word
    bool verify = true;
    // Test-only per-slot fingerprint of the last render (option "pixel_probe", akr_pixel_probe);
    // 2: completion times in the probe (counting build, diagnostic)
    int pixel_probe = 0;
    bool probe() const { return pixel_probe != 0; }
    bool probe_clock() const { return pixel_probe == 2; }
    bool fault_test = false;  // option "fault_test": k_path_defer raises the fault word once (tests)
    // option "film_variance" (default 0, read when a session starts): the session tracks the variance of every
    // slot's mean from its passes (k_variance_update after each call that draws samples).
    // Off: nothing is allocated or launched
    bool film_variance = false;
    // option "mis" (default 0, read when a session starts): direct lighting is the power-heuristic combination
    // of the next-event sample and the BSDF sample; the render takes the wavefront form.
    // Off: nothing is allocated, and every launch is the one it was
    bool mis = false;
    // option "env_path" (default 0, read at every render and continue, like "path"): an environment light no
    // longer forces the wavefront form; where the rule of "path" takes a persistent kernel, k_path's environment
    // build renders the scene (k_path_env), bit for bit what k_shade_env gives.
    // Off: every launch is the one it was
    bool env_path = false;
    // option "env_forms" (default 0, read at every render and continue): with an environment set and env_path 1,
    // the form rule of "path" decides as it does without an environment (path_defer / path_spec, the cache and
    // tail rules, the gated launch), and k_path_defer's / k_path_spec's environment builds carry it out
    // (k_path_defer_env, k_path_spec_env), bit for bit what k_shade_env gives.
    // Off, or env_path 0, or no environment: every launch is the one it was
    bool env_forms = false;

    // The render form of a constant-shading scene.  A "tail form"
    // (k_path_spec, or k_path_defer when path_spec is 0) pays where k_path's launch would end on a few
    // long pixel chains while most lanes idle: few pixels per resident lane, and many pixels whose
    // paths end at once (the camera ray leaves the scene), whose lanes then free up early.  Both come
    // from the render itself: pixels per resident lane from the occupancy query, the share of camera
    // rays that miss from the cost-ordering pilot (which marks them).  A render without a pilot
    // (below the order's spp floor, or path_order 0) runs k_path.
    // option "path_defer": 1 = k_path_defer (max_depth <= 8), 0 = k_path, 2 (default) = the rule above
    int path_defer = 2;
    // option "path_spec": k_path_spec (lanes left idle by the drained pixel queue run
    // later samples of a busy pixel from guessed sampler states; committed in order, bit-exact):
    // 1 = always, 0 = never (the rule's tail form is then k_path_defer), 2 (default) = the tail form
    // when path_defer is 2.  Measured on C3 at 1040 spp: 8-way share 0.89 -> 0.83 ms per spp against
    // k_path_defer, 2-way 2.55 -> 2.48 against k_path, the whole frame 5 % slower (profiles/r19_spec_*.log)
    int path_spec = 2;
    // option "path_tail_ppl10": tail forms only at most path_tail_ppl10 / 10 pixels per resident lane
    // (default 6.0).  1080p C3 on one MI355X: the whole frame has 7.9 pixels per lane (k_path 4.61 ms
    // against 4.85 for k_path_spec), a 2-way share 4.0 (2.55 against 2.48)
    int64_t path_tail_ppl10 = 60;
    // option "path_tail_steps": ... and a cost-ordering pilot whose camera rays take at least this many
    // traversal steps (wide-node visits + triangle tests) on average: long dependent-fetch chains, where
    // a lane freed early can run work that overlaps them (DESIGN.md §3.12 gives the measured means of
    // the soup's and the Cornell box's shares; the box's rays are a few steps long, its shares run k_path)
    int path_tail_steps = 12;
    // option "path_cache_mb": a BVH of at most this many MiB on the device (wide nodes + leaf blob) is
    // taken as cache-resident (half the 256-MiB Infinity Cache: the kernel streams its film and rays
    // beside it, MI355X_MICROARCH.md §Infinity Cache): its rule form is k_path_defer at every size
    // (the SBVH of a 100K-triangle soup is 10.7 MiB and of a 1M soup 109.8 MiB: both cache-resident,
    // k_path_defer 4-20 % faster than k_path there; the 10M soup's 1.5 GB tree takes k_path_spec on
    // rank shares)
    int64_t path_cache_mb = 128;
    // explicit overrides of the rule's size test (0, default: pixels per lane): a tail form for renders
    // of at most this many pixels (options "path_spec_pixels", "path_defer_pixels"); option
    // "path_defer_min_tris" (0, default: no test) keeps scenes below it on k_path
    int64_t path_spec_pixels = 0;
    int64_t path_defer_pixels = 0;
    int64_t path_defer_min_tris = 0;
    int path_spec_fetch = 3;   // option "path_spec_fetch": k_path_spec's ordered fetch, FETCH_STRIDE (3); -1 = the path_order_pair rule
    // ... for renders of at most 1.5 pixels per resident lane (the 8-way share) or, when set, at most
    // path_spec_fetch_pixels pixels; larger ones (2- and 4-way) take the path_order_pair rule: 2.500 /
    // 1.399 ms against 2.526 / 1.403 strided (profiles/r20_spec_fetch_ab.log)
    int64_t path_spec_fetch_pixels = 0;
    int path_spec_depth = 3;   // option "path_spec_depth": samples in flight beyond a pixel's head (1-3, the
                               // speculation tree's levels; the r19 main line measured 2, 4, 8, 15 alike, 1 slower,
                               // profiles/r19_spec_depth.log)
    bool path_mix = true;     // option "path_mix": k_path_defer fetches pixels in scrambled order
    bool path_tab = true;     // option "path_tab": persistent kernels read the scene tables from an LDS copy
    // option "path_order": cost-ordered pixel fetch: a pilot camera ray per pixel
    // ranks the pixels, and each XCD shard hands out its costliest pixels first, so a launch ends on
    // cheap ones (in k_path_defer it replaces the scrambled fetch).  2 (default) = both persistent
    // kernels, 1 = k_path only, 0 = off; renders of at least path_order_min_spp samples only (the
    // pilot costs about one third of a sample pass); classes
    // of 2^path_order_shift pilot steps.  Measured on C3 at 64 spp: 2- / 4- / 8-way shares 2-5 % faster
    int path_order = 2;
    // option "path_order_pair": the cost-ordered fetch of k_path_defer pairs each shard's costliest
    // pixels with its cheapest inside a wave (lanes done early take the long pixels' shadow rays)
    // instead of costliest-first: 1 = on, 0 = off, 3 = on for k_path too, 2 (default) = on for renders of at most
    // 1.5 pixels per resident lane (the 8-way share of a 1080p frame; measured on C3 at 32 spp, DESIGN.md §3.10: 8-way share 1.007 -> 0.946 ms, 4-way share
    // 1.499 -> 1.548 ms); option "path_prio": waves whose pixels lie in the first path_prio / 256 of
    // a cost-ordered shard run at raised issue priority (0 = off; measured without effect)
    int path_order_pair = 2;
    int path_prio = 0;
    // (16: at the driver's 20 spp the order makes the whole 1080p C3 frame 1.6 % faster, pilot included:
    // 4.905 -> 4.826 ms per spp, three alternating runs each, profiles/r18_order_min_spp_ab.log; it was 64
    // until the leaf phase fetched two triangles with the header)
    int path_order_min_spp = 16;
    // renders of at most path_order_share_pixels pixels (a rank's share of a 2-, 4- or 8-way split)
    // take the order from path_order_share_min_spp samples: the pilot's cost shrinks with the pixel
    // count and the launch tail it shortens does not (C3 at 20 spp, DESIGN.md §3.10: 2- / 4- / 8-way
    // shares 1.5 / 4.5 / 3 % faster with the order, the whole frame unchanged)
    int64_t path_order_share_pixels = 1200000;
    int path_order_share_min_spp = 16;
    int path_order_shift = 2;
    // option "path_order_classes": at most this many cost classes (1..32), the costliest holding every
    // pixel above; fewer classes keep more of the tile order inside a shard (16 since r20: whole frame
    // 4.612 against 4.627 ms per spp, 8-way share 0.803 against 0.808, profiles/r20_order_classes_ab.log)
    int path_order_classes = 16;
    // option "path_order_cap": a pilot ray stops after this many steps (0: none); its cost class is
    // then the cap's.  The pilot is a small latency-bound launch whose length is set by its slowest
    // ray, while the order only needs coarse classes (soup against background).
    int path_order_cap = 64;
    // option "path_order_sub": one pilot ray per 2^path_order_sub slots (neighbours in a tile row
    // share its cost); 0 = a pilot ray per slot
    int path_order_sub = 0;
    // option "path_order_pilot_spp": S > 0 ranks slots by the rays their first S samples take in a
    // counting k_path render (a path pilot; nothing of it reaches the film or the sampler states)
    // instead of one pilot camera ray's steps (0, default)
    int path_order_pilot_spp = 0;
    // option "wave_order": the wavefront's camera rays queued in the cost order (costliest first in
    // each shard of the closest-hit launch), by the same rule and floors as the persistent kernels
    bool wave_order = true;
    // option "path": 1 = render with k_path, 0 = the wavefront kernels, 2 (default) = k_path when the
    // render has at most path_auto_pixels pixels (default: any size; measured on C3, DESIGN.md §3.8,
    // k_path is 5 % faster than the wavefront on a whole 1080p frame and 19-31 % faster on 2-, 4- and
    // 8-way shares)
    int path_kernel = 2;
    int64_t path_auto_pixels = INT64_MAX;
    bool path_auto_complex = false;  // option "path_auto_complex": auto also takes k_path for complex shading
    bool serial_shadow = false;  // option "serial_shadow": wavefront shadow traces on the main stream (isolated timing)
    bool any_far_first = false;  // option "any_far_first": shadow traversal visits far slots first (measured: more visits on C3)
    // option "path_min_wait": a persistent kernel's wave processes its waiting lanes once this many of
    // 64 wait (scaled to the wave's live lanes); 0 (default) = 40 (measured on C3, DESIGN.md §3.8: with
    // the paired order the 8-way share runs 0.944-0.948 ms at 40, 0.972 at 32, 1.007 at 56)
    int path_min_wait = 0;
    // options "path_pop_rounds" / "path_pop_keep" (k_path, DESIGN.md §3.1 "bounded pop"): an iteration's pop
    // site runs rounds while at least path_pop_keep lanes are unserved, at most path_pop_rounds of them; the
    // lanes left retry in the next iteration.  255 / 1 waits for the slowest lane, as stack_pop does.
    // Swept over {1, 2, 3} x {1, 4, 8, 16} on C3: the whole frame runs 3.90-3.93 ms per spp at 2 / 4 and
    // 3.91-3.92 at 3 / 4 against 4.05-4.09 for the parent and for 255 / 1 (profiles/r28_pop_sweep.log)
    int path_pop_rounds = 2, path_pop_keep = 4;
    int path_grid_pct = 100;  // option "path_grid_pct": persistent path grid as a percentage of the resident maximum

    // instrumentation
    // option "stats": 1: every kernel; 2: the dominant kernel (trace_closest, or path) only (HIP events on
    // every launch cost ~7 % at small ranks)
    int stats = 0;
    bool stats_on() const { return stats != 0; }
    bool stats_closest_only() const { return stats == 2; }
    bool count = false;       // option "count_tests": the counting kernel builds
    bool exact_cull = false;  // true: the reference intersectAABB (no behind-origin cull)
    int rays_per_lane = 1;    // trace grid sizing: at least this many queued rays per lane
    // persistent shadow-trace grid as a percentage of the resident maximum: the shadow trace runs beside
    // the next closest-hit trace, and 75 % leaves it room (wavefront 5.368 / 5.353 ms per spp against
    // 5.400 / 5.389 at 100 %, 5.395 / 5.380 at 50 %; profiles/r20_shadow_grid_ab.log)
    int shadow_grid_pct = 75;
    bool wide = true;         // 4-wide quantized traversal (false: BVH2 kernel only, for A/B)
    bool lean = true;         // fused per-node slot-test arithmetic (kernels.hip visit_wide_lean; false: A/B)
    // option "leaf_align" (taken by the next build or import): each leaf record of the device blob
    // starts on a multiple of this many 16-B words (1 = packed; 8 = a 128-B line, so a leaf of at
    // most two triangles is one fabric request and the leaf phase's eight-load batch never straddles
    // two lines, tools/fetch_calib: a straddling 128-B gather costs 1.4 requests per line)
    int leaf_align = 1;
    bool ray_steps = false;   // diagnostic: standalone traces record per-ray iterations (counted kernel)
    // option count_lines (counting build, k_path, with count_tests): the bitmap of 128-B lines a render read
    bool count_lines = false;
};

// A row of the option table: an option's name, its field, and the values it takes.  FLAG: any, non-zero is
// true.  RANGE: an integer in [lo, hi].  FLOOR: the same, stored clamped to INT32_MAX.  POW2: a power of two
// in [lo, hi].  TRI: any; 2 stays 2 and every other non-zero value is 1 (Options::stats_on() and its like
// derive the field's two booleans).
constexpr int64_t kOptMin = INT64_MIN, kOptMax = INT64_MAX;
struct OptionRow {
    enum Kind { FLAG, RANGE, FLOOR, POW2, TRI };
    const char *name;
    Kind kind;
    int64_t lo, hi;
    bool Options::*b = nullptr;
    int Options::*i = nullptr;
    int64_t Options::*l = nullptr;
    constexpr OptionRow(const char *n, bool Options::*f) : name(n), kind(FLAG), lo(kOptMin), hi(kOptMax), b(f) {}
    constexpr OptionRow(const char *n, int Options::*f, int64_t lo_, int64_t hi_, Kind k = RANGE)
        : name(n), kind(k), lo(lo_), hi(hi_), i(f) {}
    constexpr OptionRow(const char *n, int64_t Options::*f, int64_t lo_, int64_t hi_) : name(n), kind(RANGE), lo(lo_), hi(hi_), l(f) {}
};

inline constexpr OptionRow kOptionTable[] = {
    {"stats", &Options::stats, kOptMin, kOptMax, OptionRow::TRI},
    {"exact_cull", &Options::exact_cull},
    {"count_tests", &Options::count},
    {"count_lines", &Options::count_lines},
    {"ray_steps", &Options::ray_steps},
    {"wide", &Options::wide},
    {"lean", &Options::lean},
    {"shadow_grid_pct", &Options::shadow_grid_pct, 1, 100},
    {"path", &Options::path_kernel, 0, 2},  // 0 (wavefront), 1 (path kernel) or 2 (auto)
    {"path_auto_complex", &Options::path_auto_complex},
    {"path_auto_pixels", &Options::path_auto_pixels, 0, kOptMax},
    {"serial_shadow", &Options::serial_shadow},
    {"any_far_first", &Options::any_far_first},
    {"path_defer", &Options::path_defer, 0, 2},  // 2: auto
    {"path_defer_min_tris", &Options::path_defer_min_tris, 0, kOptMax},
    {"path_defer_pixels", &Options::path_defer_pixels, 0, kOptMax},
    {"path_order", &Options::path_order, 0, 2},
    {"path_order_min_spp", &Options::path_order_min_spp, 0, kOptMax, OptionRow::FLOOR},
    {"path_order_share_pixels", &Options::path_order_share_pixels, 0, kOptMax},
    {"path_order_share_min_spp", &Options::path_order_share_min_spp, 0, kOptMax, OptionRow::FLOOR},
    {"path_order_cap", &Options::path_order_cap, 0, INT32_MAX},
    {"path_order_sub", &Options::path_order_sub, 0, 5},
    {"path_order_classes", &Options::path_order_classes, 1, 32},
    {"path_order_shift", &Options::path_order_shift, 0, 31},
    {"path_order_pair", &Options::path_order_pair, 0, 3},  // 2: auto, 3: both persistent kernels
    {"path_prio", &Options::path_prio, 0, 256},
    {"path_mix", &Options::path_mix},
    {"path_tab", &Options::path_tab},
    {"path_spec", &Options::path_spec, 0, 2},
    {"wave_order", &Options::wave_order},
    {"path_order_pilot_spp", &Options::path_order_pilot_spp, 0, 64},
    {"path_spec_depth", &Options::path_spec_depth, 1, 3},
    {"path_spec_fetch_pixels", &Options::path_spec_fetch_pixels, 0, kOptMax},
    {"path_spec_fetch", &Options::path_spec_fetch, -1, 3},
    {"path_tail_ppl10", &Options::path_tail_ppl10, 0, kOptMax},
    {"leaf_align", &Options::leaf_align, 1, 8, OptionRow::POW2},
    {"path_cache_mb", &Options::path_cache_mb, 0, kOptMax},
    {"path_tail_steps", &Options::path_tail_steps, 0, 4096},
    {"path_spec_pixels", &Options::path_spec_pixels, 0, kOptMax},
    {"path_grid_pct", &Options::path_grid_pct, 1, 100},
    {"path_min_wait", &Options::path_min_wait, 0, 64},  // 0: per kernel
    {"path_pop_rounds", &Options::path_pop_rounds, 1, 255},
    {"path_pop_keep", &Options::path_pop_keep, 1, 64},
    {"pixel_probe", &Options::pixel_probe, kOptMin, kOptMax, OptionRow::TRI},
    {"fault_test", &Options::fault_test},
    {"verify", &Options::verify},
    {"rays_per_lane", &Options::rays_per_lane, 1, 64},
};

inline const OptionRow *find_option(const char *key) {
    for (const OptionRow &r : kOptionTable)
        if (key && strcmp(r.name, key) == 0) return &r;
    return nullptr;
}

// The field of `o` a row names, as an integer
inline int64_t get_option(const Options &o, const OptionRow &r) { return r.b ? (o.*r.b ? 1 : 0) : (r.i ? o.*r.i : o.*r.l); }

// Stores `value` under `key`.  Returns an empty string, or why the value was refused (`o` is then unchanged).
inline std::string set_option(Options &o, const char *key, int64_t value) {
    // a session switch, not a knob of the render: kOptionTable stays the record of the knobs row for row
    // (tests/golden/options.json), and this one name is matched before it
    if (key && strcmp(key, "film_variance") == 0) {
        if (value != 0 && value != 1) return "film_variance must be in [0, 1]";
        o.film_variance = value == 1;
        return {};
    }
    if (key && strcmp(key, "mis") == 0) {  // the same kind of switch
        if (value != 0 && value != 1) return "mis must be in [0, 1]";
        o.mis = value == 1;
        return {};
    }
    if (key && strcmp(key, "env_path") == 0) {  // a choice of form under an environment
        if (value != 0 && value != 1) return "env_path must be in [0, 1]";
        o.env_path = value == 1;
        return {};
    }
    if (key && strcmp(key, "env_forms") == 0) {  // which persistent forms env_path may take
        if (value != 0 && value != 1) return "env_forms must be in [0, 1]";
        o.env_forms = value == 1;
        return {};
    }
    const OptionRow *r = find_option(key);
    if (!r) return "unknown option '" + std::string(key ? key : "") + "'";
    const bool pow2 = r->kind == OptionRow::POW2;
    if (value < r->lo || value > r->hi || (pow2 && (value & (value - 1)) != 0))
        return std::string(key) + " must be in [" + std::to_string(r->lo) + ", " + std::to_string(r->hi) + "]" +
               (pow2 ? " and a power of two" : "");
    if (r->kind == OptionRow::FLAG) o.*r->b = value != 0;
    else if (r->kind == OptionRow::TRI) o.*r->i = value == 2 ? 2 : (value != 0 ? 1 : 0);
    else if (r->l) o.*r->l = value;
    else o.*r->i = (int)(value < INT32_MAX ? value : INT32_MAX);  // only a FLOOR row's hi lies above INT32_MAX
    return {};
}

}  // namespace akr

// path_build.h — which build of the persistent path kernels a launch runs, and the names of
// the wavefront shade kernels' builds.  Plain C++, no HIP header: kernels.hip maps a key to its kernel, capi.hip
// keeps one grid per key, tests/cpp/path_build_check.cpp pins the rule.
#pragma once
#include "akr_path_forms.h"

namespace akr {

struct PathBuild {
    int kind;       // PATH_PLAIN / PATH_DEFER / PATH_SPEC
    bool count;     // the counting build (ray tallies, probes)
    bool tab;       // the shading tables in LDS
    bool leaf_one;  // PATH_PLAIN's one-triangle leaf phase
    bool simple;    // the shading for tables of constant Diffuse / Emissive (shade_simple.h)
    bool env;       // the environment twin of the same build
};

// The key of the kernel that runs for `b`: several keys share one.  The counting builds shade with the general
// build and have no one-triangle leaf phase; only PATH_PLAIN has that phase, and only with the simple shading
// (k_path<false, TAB>): every other PATH_PLAIN product build is a k_path_general, whose leaf phase finds the
// same hits.
inline PathBuild canonical(PathBuild b) {
    if (b.count) b.simple = false;
    if (b.kind != PATH_PLAIN || !b.simple) b.leaf_one = false;
    return b;
}

// 20 kernels without an environment and their 20 twins with one (the table in DESIGN.md §0.5)
constexpr int kPathBuilds = 40;

// A dense index of canonical(b): [0, 6) the counting builds, [6, 14) PATH_DEFER's and PATH_SPEC's product
// builds, [14, 20) PATH_PLAIN's (per tab: general shading, simple, simple with the one-triangle leaf phase);
// + 20 with an environment
inline int build_index(PathBuild b) {
    static_assert(PATH_PLAIN == 0 && PATH_DEFER == 1 && PATH_SPEC == 2, "the index counts the kinds from 0");
    b = canonical(b);
    int i;
    if (b.count) i = b.kind * 2 + b.tab;
    else if (b.kind != PATH_PLAIN) i = 6 + (b.kind - 1) * 4 + b.tab * 2 + b.simple;
    else i = 14 + b.tab * 3 + b.simple + b.leaf_one;
    return b.env ? i + kPathBuilds / 2 : i;
}

// the wavefront shade kernel's builds: k_shade[_env][_spec][_mis]
struct ShadeBuild {
    bool env, mis, spec;
};

}  // namespace akr

// Drives csrc/path_build.h for tests/test_path_build_host.py.  Takes no input: walks all 96 keys (3 kinds x 2^5
// flags), checks every rule of canonical() and build_index() by name, and prints one line per key:
//   <kind> <count> <tab> <leaf_one> <simple> <env> -> <the canonical key's six fields> <build_index>
// A broken rule prints "FAIL <rule>: <key>" and the exit status is 1.
#include <cstdio>

#include "path_build.h"

using akr::PathBuild;

static int g_fail = 0;
static void check(bool ok, const char *rule, const PathBuild &b) {
    if (ok) return;
    g_fail++;
    std::printf("FAIL %s: %d %d %d %d %d %d\n", rule, b.kind, b.count, b.tab, b.leaf_one, b.simple, b.env);
}
static bool same(const PathBuild &a, const PathBuild &b) {
    return a.kind == b.kind && a.count == b.count && a.tab == b.tab && a.leaf_one == b.leaf_one && a.simple == b.simple &&
           a.env == b.env;
}

int main() {
    static_assert(akr::kPathBuilds == 40, "20 kernels and their environment twins");
    int owners = 0;                          // canonical keys met
    bool taken[akr::kPathBuilds] = {};       // indices some canonical key has
    for (int kind = 0; kind < 3; kind++)
        for (int f = 0; f < 32; f++) {
            const PathBuild b{kind, (f & 16) != 0, (f & 8) != 0, (f & 4) != 0, (f & 2) != 0, (f & 1) != 0};
            const PathBuild c = akr::canonical(b);
            const int i = akr::build_index(b);
            check(same(akr::canonical(c), c), "canonical is idempotent", b);
            check(c.kind == b.kind && c.count == b.count && c.tab == b.tab, "kind, count and tab are kept", b);
            check(c.env == b.env, "env is kept", b);
            if (b.count) check(!c.simple && !c.leaf_one, "a counting build runs the general shading, no leaf_one", b);
            if (b.kind != akr::PATH_PLAIN) check(!c.leaf_one, "only PATH_PLAIN has leaf_one", b);
            if (b.kind == akr::PATH_PLAIN && !b.simple) check(!c.leaf_one, "general shading of PATH_PLAIN has no leaf_one", b);
            if (!b.count) check(c.simple == b.simple, "a product build keeps simple", b);
            if (b.kind == akr::PATH_PLAIN && !b.count && b.simple)
                check(c.leaf_one == b.leaf_one, "simple PATH_PLAIN keeps leaf_one", b);
            check(i >= 0 && i < akr::kPathBuilds, "the index is in range", b);
            check(i == akr::build_index(c), "a key has its canonical key's index", b);
            const PathBuild twin{b.kind, b.count, b.tab, b.leaf_one, b.simple, !b.env};
            check(akr::build_index(twin) == (b.env ? i - 20 : i + 20), "env selects the twin 20 further", b);
            if (same(b, c) && i >= 0 && i < akr::kPathBuilds) {
                check(!taken[i], "canonical keys have distinct indices", b);
                taken[i] = true;
                owners++;
            }
            std::printf("%d %d %d %d %d %d -> %d %d %d %d %d %d %d\n", b.kind, b.count, b.tab, b.leaf_one, b.simple, b.env, c.kind,
                        c.count, c.tab, c.leaf_one, c.simple, c.env, i);
        }
    if (owners != akr::kPathBuilds) {
        g_fail++;
        std::printf("FAIL the canonical keys fill [0, 40): %d\n", owners);
    }
    return g_fail ? 1 : 0;
}

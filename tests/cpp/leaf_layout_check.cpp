// Drives csrc/leaf_layout.h for tests/test_leaf_layout_host.py.  Each input line is
//   <align> <count> <count> ...        or        <align> repeat <n_leaves> <count>        or        pays <n_one> <n_leaves>
// and the reply is one line: "words=<W> pad=<P> <offset>:<ref in hex> ..." (the second form prints only
// the last leaf's pair), "error <message>", or for the third form leaf_one_pays() as 0 or 1.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "leaf_layout.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.rfind("pays ", 0) == 0) {
            std::istringstream q(line.substr(5));
            size_t n_one = 0, n_leaves = 0;
            q >> n_one >> n_leaves;
            std::printf("%d\n", akr::leaf_one_pays(n_one, n_leaves) ? 1 : 0);
            continue;
        }
        std::istringstream in(line);
        size_t align = 0;
        std::string tok;
        in >> align;
        std::vector<uint64_t> counts;
        size_t n = 0;
        uint64_t each = 0;
        bool repeat = false;
        while (in >> tok) {
            if (tok == "repeat") {
                repeat = true;
                in >> n >> each;
                break;
            }
            counts.push_back(std::stoull(tok));
        }
        if (!repeat) n = counts.size();
        auto count = [&](size_t i) { return repeat ? each : counts[i]; };
        try {
            const akr::LeafLayout l = akr::leaf_layout(n, align, count);
            std::printf("words=%zu pad=%zu", l.words, akr::kLeafBlobPad);
            for (size_t i = repeat && n ? n - 1 : 0; i < n; i++)
                std::printf(" %u:%08x", l.offset[i], l.ref(i, (uint32_t)count(i)));
            std::printf("\n");
        } catch (const std::exception &e) {
            std::printf("error %s\n", e.what());
        }
    }
    return 0;
}

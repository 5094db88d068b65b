// Drives csrc/tile_layout.h for tests/test_session_host.py.  Each input line is
//   <W> <H> <pixels: 0 or 1> <n_tiles> <x0> <y0> <x1> <y1> ...
// and the reply is one line: "n=<slots> alloc=<bytes layout_tiles allocated> tiles=<x0>,<y0>,<width>,<first>;...
// px=<packed pixel of every slot in hex>,... frame=<frame_index of every slot>,..." (px and frame only when
// asked for), or "error <message>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include "tile_layout.h"

static size_t g_alloc = 0;
void *operator new(size_t n) {
    g_alloc += n;
    if (void *p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void operator delete(void *p) noexcept { std::free(p); }
void operator delete(void *p, size_t) noexcept { std::free(p); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int W = 0, H = 0, pixels = 0, n = 0;
        in >> W >> H >> pixels >> n;
        std::vector<akr_rect> tiles(n);
        for (akr_rect &t : tiles) in >> t.x0 >> t.y0 >> t.x1 >> t.y1;
        try {
            const size_t before = g_alloc;
            const akr::TileLayout l = akr::layout_tiles(tiles.data(), n, W, H, "render call");
            const size_t used = g_alloc - before;
            std::printf("n=%llu alloc=%zu tiles=", (unsigned long long)l.n, used);
            for (const akr::TileRec &t : l.tiles) std::printf("%u,%u,%u,%u;", t.x0, t.y0, t.width, t.first);
            if (pixels) {
                std::vector<uint32_t> px;
                akr::slot_pixels(l, px);
                std::printf(" px=");
                for (uint32_t p : px) std::printf("%x,", p);
                std::printf(" frame=");
                for (uint32_t p : px) std::printf("%llu,", (unsigned long long)akr::frame_index(p, W));
            }
            std::printf("\n");
        } catch (const std::exception &e) {
            std::printf("error %s\n", e.what());
        }
    }
    return 0;
}

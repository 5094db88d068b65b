// tile_layout.h — how a tile list becomes film slots: plain C++, no HIP, so the rule is
// checked on the CPU (tests/cpp/tile_layout_check.cpp).  Every render, feature pass and state import lays
// its tiles out here; every host-side merge reads its slots' pixels from here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/akr_hip.h"  // akr_rect

namespace akr {

// One clipped, non-empty tile as the device reads it (a uint4: k_expand_pixels)
struct alignas(16) TileRec {
    uint32_t x0, y0, width, first;  // first: the slot of the tile's top-left pixel
};

struct TileLayout {
    std::vector<TileRec> tiles;
    uint64_t n = 0;  // slots: the tiles' pixels, tiles in order, row-major inside a tile
};

constexpr uint64_t kMaxSlots = 1ull << 31;

// The tiles clipped to the W x H frame, empty ones skipped, each with its first slot.  A list of 2^31 slots
// or more is refused: "too many pixels in one <what>".  Nothing is allocated per pixel.
inline TileLayout layout_tiles(const akr_rect *tiles, int32_t n_tiles, int32_t W, int32_t H, const char *what) {
    TileLayout l;
    for (int32_t k = 0; k < n_tiles && l.n < kMaxSlots; k++) {
        const int x0 = std::max(0, tiles[k].x0), y0 = std::max(0, tiles[k].y0);
        const int x1 = std::min(W, tiles[k].x1), y1 = std::min(H, tiles[k].y1);
        if (x1 <= x0 || y1 <= y0) continue;
        l.tiles.push_back({(uint32_t)x0, (uint32_t)y0, (uint32_t)(x1 - x0), (uint32_t)l.n});
        l.n += (uint64_t)(x1 - x0) * (uint64_t)(y1 - y0);
    }
    if (l.n >= kMaxSlots) throw std::runtime_error(std::string("too many pixels in one ") + what);
    return l;
}

// Every slot's pixel, packed x | y << 16 (the frame is at most 65535 wide and high)
inline void slot_pixels(const TileLayout &l, std::vector<uint32_t> &out) {
    out.resize(l.n);
    for (size_t k = 0; k < l.tiles.size(); k++) {
        const TileRec &t = l.tiles[k];
        const uint64_t end = k + 1 < l.tiles.size() ? l.tiles[k + 1].first : l.n;
        for (uint64_t i = t.first; i < end; i++) {
            const uint32_t local = (uint32_t)(i - t.first);
            out[i] = (t.x0 + local % t.width) | ((t.y0 + local / t.width) << 16);
        }
    }
}

// A packed pixel's index in the row-major frame of width W
inline uint64_t frame_index(uint32_t px, int32_t W) { return (uint64_t)(px & 0xFFFFu) + (uint64_t)(px >> 16) * (uint64_t)W; }

}  // namespace akr

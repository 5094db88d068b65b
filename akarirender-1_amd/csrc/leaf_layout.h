// leaf_layout.h — where each leaf of the wide view lies in the device leaf blob, and the reference a wide
// node holds to it.  A leaf's record is two float4 of header followed by three float4 per triangle; a
// device leaf reference is AKR_CHILD_LEAF | flags | the record's float4 offset.  Plain C++, no HIP header:
// capi.hip's finish_accel() lays the blob out with it, tests/cpp/leaf_layout_check.cpp exercises it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <vector>

#include "../../include/akr_bvh_format.h"

namespace akr {

// Bit 30 of a device leaf reference: the leaf holds exactly one triangle (kernels.hip path_leaf).
// AKR_CHILD_EMPTY and the kernels' AKR_CHILD_POP carry the bit too: only a leaf holder's reference says it.
constexpr uint32_t kLeafOne = 1u << 30;
constexpr uint32_t kLeafOffsetMask = kLeafOne - 1u;  // the offset: 30 bits, 16 GB of blob
// zero float4 behind the last leaf: a leaf phase may fetch the second triangle record with the header
// whatever the leaf's count
constexpr size_t kLeafBlobPad = 3;

// Whether k_path's leaf phase for one-triangle leaves (kernels.hip path_leaf_masks) is worth running on a
// tree with n_one one-triangle leaves among n_leaves.  The phase's block runs only in a wave none of whose
// leaf holders lacks the flag; any other wave pays the phase's entry on top of the general form, and on a
// scene of mixed leaves with coherent rays the general form's early returns beat the block (the Cornell
// box: 1.2 % slower with it).  A leaf phase has about 22 holders: with a share p of
// flagged leaves about p^22 of the phases are the block, and at least half of them are from p = 0.97
// (0.97^22 = 0.51).  Below that the general kernel runs.  The C3 soup has p = 0.9995.
inline bool leaf_one_pays(size_t n_one, size_t n_leaves) { return n_leaves > 0 && n_one * 100 >= n_leaves * 97; }

struct LeafLayout {
    std::vector<uint32_t> offset;  // float4 offset of leaf i's record
    size_t words = 0;              // float4 of the blob without its padding

    // the device reference of leaf i, which holds `count` triangles
    uint32_t ref(size_t i, uint32_t count) const { return AKR_CHILD_LEAF | (count == 1 ? kLeafOne : 0u) | offset[i]; }
};

// Leaf i holds count(i) triangles; each record starts at a multiple of `align` float4.
template <class Count>
inline LeafLayout leaf_layout(size_t n_leaves, size_t align, Count count) {
    LeafLayout l;
    l.offset.resize(n_leaves);
    if (align < 1) align = 1;
    size_t words = 0;
    for (size_t i = 0; i < n_leaves && words < kLeafOne; i++) {
        words = (words + align - 1) / align * align;
        if (words >= kLeafOne) break;
        l.offset[i] = (uint32_t)words;
        words += 2 + 3 * (size_t)count(i);
    }
    if (words >= kLeafOne)
        throw std::runtime_error("BVH too large for the wide leaf blob: a leaf reference holds a 30-bit float4 offset (16 GB)");
    l.words = words;
    return l;
}

}  // namespace akr

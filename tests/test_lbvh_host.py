"""The numpy restatement of the GPU LBVH builder (tests/golden/lbvh_restate.py) against things it
shares no code with (no GPU needed): helpers.check_bvh and the library's akr_bvh_validate on its tree,
the radix-tree property of every node by brute force over the node's leaf sets, its f32 cells against
cells quantised in float64, and the depth of the chain scene on both sides of AKR_BVH_MAX_DEPTH.
tests/test_gpu_lbvh.py then holds the device's tree to this restatement byte for byte."""
import sys

import numpy as np
import pytest

from akari_amd import capi, scene
from conftest import GOLDEN
from helpers import (CHAIN_CELLS, LBVH_INPUTS, chain_cells, chain_scene, check_bvh, check_split_planes,
                     subtree_leaves)

sys.path.insert(0, str(GOLDEN))
import lbvh_restate as L  # noqa: E402

_cache = {}


def restated(name):
    """(compiled scene, nodes, tris) of an input: restated once, shared, never written."""
    if name not in _cache:
        cs = scene.compile_scene(LBVH_INPUTS[name]())
        nodes, tris = L.restate(cs.vertices, cs.indices)
        nodes.setflags(write=False)
        tris.setflags(write=False)
        _cache[name] = (cs, nodes, tris)
    return _cache[name]


def test_record_layouts():
    assert L.NODE_DTYPE == capi.NODE_DTYPE and L.TRI_DTYPE == capi.TRI_DTYPE
    assert (L.LEAF, L.EMPTY, L.CELLS) == (0x80000000, 0xFFFFFFFF, CHAIN_CELLS)


@pytest.mark.parametrize("name", list(LBVH_INPUTS))
def test_restated_tree_is_valid(name):
    """check_bvh's invariants, and the library's validator counts the depth the restatement counts."""
    cs, nodes, tris = restated(name)
    assert len(tris) == cs.n_tris and len(nodes) == cs.n_tris
    check_bvh(cs, nodes, tris, 1)
    assert capi.validate_bvh(nodes, tris, cs.n_tris) == L.depth(nodes)
    assert not nodes["_pad"].any() and not tris["_p0"].any() and not tris["_p1"].any()
    assert nodes["child"][0][1] == L.EMPTY
    assert np.all(np.isposinf(nodes[0]["bxy1"][[0, 2]])) and np.all(np.isneginf(nodes[0]["bxy1"][[1, 3]]))
    assert np.isposinf(nodes[0]["bz"][2]) and np.isneginf(nodes[0]["bz"][3])


def _top_bit(x):
    return int(x).bit_length() - 1


@pytest.mark.parametrize("name", list(LBVH_INPUTS))
def test_every_node_separates_its_leaves(name):
    """Brute force over leaf sets (gathered from the child links, not from ranges): below every internal
    node the keys (code, sorted position) agree above their highest differing bit, the left subtree's
    keys hold 0 there and the right subtree's 1, and `axis` is that bit's axis (0 when it is a bit of the
    position, the codes being all equal).  The root holds every leaf, so by induction every node is the
    full set of keys with its prefix: the tree is the radix tree of the sorted keys."""
    cs, nodes, tris = restated(name)
    codes, _, _ = L.morton(cs.vertices, cs.indices)
    gid = tris["gid"].astype(np.int64)
    assert np.all(codes[gid][1:] >= codes[gid][:-1]), "leaves are not in code order"
    order, sets = subtree_leaves(nodes)
    assert len(order) == cs.n_tris - 1
    if order:
        assert sorted(np.concatenate(sets[order[0]]).tolist()) == list(range(cs.n_tris))
    for r in order:
        left, right = sets[r]
        cl, cr = codes[gid[left]], codes[gid[right]]
        both = np.concatenate([cl, cr])
        x = int(np.bitwise_or.reduce(both ^ both[0]))
        if x:
            b = _top_bit(x)
            lo_side, hi_side, want_axis = (cl >> np.uint64(b)) & np.uint64(1), (cr >> np.uint64(b)) & np.uint64(1), 2 - b % 3
        else:
            pos = np.concatenate([left, right])
            b = _top_bit(int(np.bitwise_or.reduce(pos ^ pos[0])))
            lo_side, hi_side, want_axis = (left >> b) & 1, (right >> b) & 1, 0
        assert not lo_side.any() and hi_side.all(), f"{name}: node {r} does not split at bit {b}"
        assert nodes["axis"][r] == want_axis, f"{name}: node {r} axis {nodes['axis'][r]}, bit {b}"
    if name == "sheet":
        assert not (nodes["axis"][1:] == 2).any()
    if name == "identical":
        assert not nodes["axis"].any() and len(np.unique(codes)) == 1


@pytest.mark.parametrize("name", list(LBVH_INPUTS))
def test_f32_cells_within_one_of_f64_cells(name):
    """t = (c - lo) / ext carries a few ulp of 1 in f32, and 2^-23 * 2^21 is a quarter of a cell: the f32
    cell of a centre is the float64 cell or a neighbour.  This is the margin of the device test of the split
    planes (test_gpu_lbvh.py), asserted here for the reference alone, and that test's check run on the
    restated tree."""
    cs, nodes, tris = restated(name)
    _, q32, c32 = L.morton(cs.vertices, cs.indices)
    c64, q64 = L.code_cells_f64(cs.vertices, cs.indices)
    assert np.array_equal(c64, c32.astype(np.float64))
    d = np.abs(q64 - q32.astype(np.int64))
    print(name, "cells that differ:", int(np.count_nonzero(d)), "of", d.size, "largest difference", int(d.max()))
    assert d.max() <= 1
    assert check_split_planes(nodes, tris, q64) == []


def test_chain_scene_cells_and_depths():
    """The chain's triangles have area: their centres still fall in the intended cells, the codes are 0,
    the 63 single bits and all ones, and the tree has 64 levels with 65 triangles and 65 with 66."""
    for n in (65, 66):
        cs = scene.compile_scene(chain_scene(n))
        assert cs.n_tris == n
        codes, cells, _ = L.morton(cs.vertices, cs.indices)
        want = chain_cells(65)
        assert np.array_equal(cells[:65].astype(np.int64), want)
        assert [int(c) for c in codes[:65]] == [1 << (62 - j) for j in range(63)] + [0, (1 << 63) - 1]
        if n == 66:
            assert np.array_equal(cells[65].astype(np.int64), want[63])
        nodes, tris = L.restate(cs.vertices, cs.indices)
        assert L.depth(nodes) == n - 1
        if n == 65:
            assert capi.validate_bvh(nodes, tris, n) == 64 == L.MAX_DEPTH
        else:
            with pytest.raises(capi.AkrError):          # the validator's limit is the builder's
                capi.validate_bvh(nodes, tris, n)

"""The GPU LBVH builder's tree (csrc/lbvh.hip: k_tri_bounds, k_morton, the radix sort, k_karras,
k_refit, k_links, k_leaf_tris) against its numpy restatement (tests/golden/lbvh_restate.py, itself held
to brute-force properties by tests/test_lbvh_host.py).

Bar: byte equality.  The builder's output is a function of the mesh: a stable sort, internal node i in
record i + 1, leaves in sorted order, boxes that are minima and maxima.  helpers.check_bvh accepts any
valid tree and the oracle walks whatever tree came out, so a wrong spread mask, 20 bits per axis, y and z
interleaved the wrong way round, a split one position off, an `axis` that names the wrong Morton bit or a
stale box in a parent all render "correctly"; none of them gives these bytes.  Nothing is waited for or
retried before the comparison: k_refit's hand-off has one result.

  tree      accel_export() == restate() in every field of every record, on helpers.LBVH_INPUTS
  planes    the device's own tree against cells quantised in float64, not routed through the restatement
  depth     the chain scene: 65 triangles build to AKR_BVH_MAX_DEPTH = 64 levels and trace / render bit-exact
            against the oracle in every render form; 66 triangles are refused and leave the context usable
"""
import sys

import numpy as np
import pytest

import py_oracle
from akari_amd import capi, scene
from conftest import GOLDEN
from helpers import (LBVH_INPUTS, chain_axis_rays, chain_rays, chain_scene, check_bvh, check_probe, check_split_planes, edge_rays,
                     random_rays, small_soup)
from test_gpu_parity import _check_trace

sys.path.insert(0, str(GOLDEN))
import lbvh_restate as L  # noqa: E402

pytestmark = pytest.mark.gpu

_exports = {}


def exported(factory, name):
    """(compiled scene, nodes, tris, accel info) of an input built by the device: built once, never written."""
    if name not in _exports:
        cs = scene.compile_scene(LBVH_INPUTS[name]())
        with factory(0) as ctx:
            scene.upload_scene(ctx, cs, builder=capi.BUILDER_LBVH)
            nodes, tris = ctx.accel_export()
            info = ctx.accel_info()
        nodes.setflags(write=False)
        tris.setflags(write=False)
        _exports[name] = (cs, nodes, tris, (info.max_depth, info.max_leaf, info.n_nodes, info.n_tris))
    return _exports[name]


def assert_same_tree(nodes, tris, want_nodes, want_tris, what):
    for kind, got, want in (("node", nodes, want_nodes), ("leaf record", tris, want_tris)):
        d = L.first_difference(np.ascontiguousarray(got), np.ascontiguousarray(want))
        assert d is None, f"{what}: first differing {kind} {d[0]}, field {d[1]}: device {d[2]}, restatement {d[3]}"


@pytest.mark.parametrize("name", list(LBVH_INPUTS))
def test_tree_equals_restatement(hip_ctx_factory, name):
    cs, nodes, tris, (max_depth, max_leaf, n_nodes, n_tris) = exported(hip_ctx_factory, name)
    want_nodes, want_tris = L.restate(cs.vertices, cs.indices)
    assert nodes.dtype == L.NODE_DTYPE and tris.dtype == L.TRI_DTYPE
    assert_same_tree(nodes, tris, want_nodes, want_tris, name)
    assert max_depth == L.depth(want_nodes) and max_leaf == 1
    assert (n_nodes, n_tris) == (cs.n_tris, cs.n_tris)


@pytest.mark.parametrize("name", ["soup20000", "shifted"])
def test_split_planes_against_f64_cells(hip_ctx_factory, name):
    """The device's export alone (links, axis, gid), against the cells of the centres quantised in float64:
    below every internal node each left-subtree centre lies below the split plane plus one cell along `axis`
    and each right-subtree centre above it minus one cell (helpers.check_split_planes; the one-cell margin is
    asserted for the reference in test_lbvh_host.py).  A mistake the restatement shares with the kernels in
    the quantisation, the interleave or the axis does not pass this."""
    cs, nodes, tris, _ = exported(hip_ctx_factory, name)
    check_bvh(cs, nodes, tris, 1)
    _, cells = L.code_cells_f64(cs.vertices, cs.indices)
    bad = check_split_planes(nodes, tris, cells)
    assert not bad, f"{name}: {len(bad)} of {len(nodes) - 1} nodes do not separate their leaves at a cell plane of " \
                    f"their axis, first record {bad[0]} (axis {nodes['axis'][bad[0]]})"


# ------------------------------------------------------------------------------------------ the depth limit
FORMS = {   # options, the form render_form() must report
    "k_path": (dict(path=1, path_defer=0, path_spec=0, path_order=0, count_tests=0), "k_path"),
    "k_path_general_leaf": (dict(path=1, path_defer=0, path_spec=0, path_order=0, count_tests=1), "k_path"),
    "k_path_defer": (dict(path=1, path_defer=1, path_spec=0, path_order=0, count_tests=0), "k_path_defer"),
    "k_path_spec": (dict(path=1, path_defer=0, path_spec=1, path_order=0, count_tests=0), "k_path_spec"),
    "wavefront": (dict(path=0, path_defer=0, path_spec=0, path_order=0, count_tests=0), "wavefront"),
}
W = H = 24
TILES = [(0, 0, W, H)]
BESIDE_ORIGIN = (2.0 ** -23, 2.0 ** -24, 2.0 ** -25)   # inside the box of every triangle's off-axis extents (h >= 2^-22)


class Chain:
    def __init__(self, factory):
        self.cs = scene.compile_scene(chain_scene(65, (W, H)))
        self.ctx = factory(0)
        scene.upload_scene(self.ctx, self.cs, builder=capi.BUILDER_LBVH)
        self.nodes, self.tris = self.ctx.accel_export()
        self.orc = py_oracle.OracleScene(self.cs, self.nodes, self.tris, capi)
        self._ref = None

    def ref(self):
        """The oracle's 24 x 24, 2-spp, depth-5 render with its probe: computed once, never written."""
        if self._ref is None:
            rad, w, _, probe = self.orc.render(2, 5, tiles=TILES, probe=True)
            for a in (rad, w, probe):
                a.setflags(write=False)
            self._ref = (rad, w, probe)
        return self._ref


@pytest.fixture(scope="module")
def chain(hip_ctx_factory):
    c = Chain(hip_ctx_factory)
    yield c
    c.ctx.close()


def test_chain_builds_to_the_depth_limit(chain):
    """65 triangles: accepted, 64 levels, and the restatement's bytes."""
    info = chain.ctx.accel_info()
    assert info.max_depth == 64 == L.MAX_DEPTH and info.max_leaf == 1
    want_nodes, want_tris = L.restate(chain.cs.vertices, chain.cs.indices)
    assert_same_tree(chain.nodes, chain.tris, want_nodes, want_tris, "chain65")
    check_bvh(chain.cs, chain.nodes, chain.tris, 1)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("any_hit", [False, True])
def test_chain_traces(chain, any_hit, exact):
    """Closest-hit and any-hit traces of the 64-level tree against the oracle: rays along the chain's
    diagonal in both directions (inside every box of the chain), rays aimed at every triangle, edge rays.

    Why the traversal stacks hold.  A BVH2 of 64 levels has at most 63 levels of internal nodes.  The wide
    collapse (bvh_wide.cpp) makes a wide node from a treelet of one to three BVH2 internal nodes; its slots
    are the treelet's frontier children, one more than the treelet has nodes, at most four.  A visit
    continues with one entered slot and pushes the others, so it pushes at most as many entries as its
    treelet has internal nodes.  Below the root every internal node of the chain has one leaf child and one
    internal child (the root's other child is a node of two leaves), so the wide nodes lie on one path, their
    treelets are disjoint, and whatever treelets the SAH collapse chooses the entries pushed along the path,
    which bound the stack pointer at any moment, number at most the tree's internal nodes: 64.  That is below
    kStackMax = 96 (akr_device.h), the rows a lane owns: kStackLds in LDS and kStackMax - kStackLds in the
    global overflow area that capi.hip reserves per resident lane.  Rays that leave the wide traversal
    (visit_node, the exact-cull path) and the oracle walk the BVH2 itself and push one entry per level: at
    most 63, the oracle's stack holding AKR_BVH_MAX_DEPTH + 8.  So the bound holds for this tree in every
    kernel."""
    gh, oh = _check_trace(chain.ctx, chain.orc, chain.cs, chain_rays(), any_hit, exact)
    # the aimed rays hit the triangles large enough for the triangle test's determinant bound (about 30 of
    # the 65, 16 rays each), the diagonal ones the far triangle
    assert np.count_nonzero(oh["gid"] != 0xFFFFFFFF) > 400
    assert oh["gid"][0] != 0xFFFFFFFF and oh["gid"][1] != 0xFFFFFFFF
    _check_trace(chain.ctx, chain.orc, chain.cs, edge_rays(BESIDE_ORIGIN), any_hit, exact)
    _check_trace(chain.ctx, chain.orc, chain.cs, chain_axis_rays(), any_hit, exact)
    chain.ctx.set_option("exact_cull", 0)


def test_chain_rays_leave_the_lds_stack(chain):
    """A ray a hair off +x from beside the origin (helpers.chain_axis_rays; tmin 0, every 1 / d finite, so it
    stays in the wide traversal, which edge_rays' axis-parallel rays leave) enters the boxes of all 21
    triangles on the x axis and, x being their nodes' split axis and the rest of the chain the lower child,
    reaches the bottom of the chain with every one of them stacked: more than the kStackLds = 15 rows in LDS,
    so the overflow rows are used (the counting build's deep_rays).  Likewise along +y and +z."""
    rays = chain_axis_rays()
    ctx = chain.ctx
    ctx.set_option("count_tests", 1)
    ctx.reset_stats()
    try:
        _check_trace(ctx, chain.orc, chain.cs, rays, False)
        deep = ctx.trace_counts()["per_mode"]["closest"]["deep_rays"]
    finally:
        ctx.set_option("count_tests", 0)
        ctx.reset_stats()
    print(f"deep-stack rays: {deep} of {len(rays)}")
    assert deep > 0, "no ray reached the overflow stack"


@pytest.mark.parametrize("form", list(FORMS))
def test_chain_renders(chain, form):
    """24 x 24, 2 spp, depth 5 on the 64-level tree in every render form, each against the oracle with the
    probe.  Every leaf of an LBVH tree holds one triangle, so the library runs k_path with the one-triangle
    leaf phase there; the kernel without it (k_path_general) is chosen by the tree's share of such leaves
    (leaf_layout.h leaf_one_pays), which no option overrides.  Its leaf phase, the general form, runs on this
    tree in k_path's counting build (count_tests), which also records the per-pixel ray counts."""
    opts, want_form = FORMS[form]
    ctx = chain.ctx
    orad, ow, oprobe = chain.ref()
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_option("pixel_probe", 1)
    try:
        rad, w = ctx.render(2, 5, TILES, W, H)
        assert ctx.render_form()["form"] == want_form
        assert np.array_equal(w, ow)
        assert np.array_equal(rad, orad), f"{form}: {np.count_nonzero(rad != orad)} radiance values differ"
        rays = check_probe(ctx.pixel_probe(W * H), oprobe, TILES, W, H, form)
        assert rays == (form in ("wavefront", "k_path_general_leaf"))
    finally:
        ctx.set_option("pixel_probe", 0)
        ctx.set_option("count_tests", 0)
    assert np.all(w == 2) and rad.mean() > 0


def test_one_level_too_deep_is_refused(hip_ctx_factory):
    """66 triangles (the origin triangle doubled): 65 levels, refused with the builder's message.  The same
    context then takes the 37-triangle soup (akr_hip_clear_meshes: uploads append), builds it with the same
    builder and traces it bit-exact: a refused build leaves the context usable."""
    deep = scene.compile_scene(chain_scene(66))
    assert L.depth(L.restate(deep.vertices, deep.indices)[0]) == 65
    with hip_ctx_factory(0) as ctx:
        with pytest.raises(capi.AkrError, match="deeper than"):
            scene.upload_scene(ctx, deep, builder=capi.BUILDER_LBVH)
        with pytest.raises(capi.AkrError):
            ctx.accel_info()                       # no tree was adopted
        ctx.clear_meshes()
        cs = scene.compile_scene(small_soup(37))
        scene.upload_scene(ctx, cs, builder=capi.BUILDER_LBVH)
        nodes, tris = ctx.accel_export()
        want_nodes, want_tris = L.restate(cs.vertices, cs.indices)
        assert_same_tree(nodes, tris, want_nodes, want_tris, "soup after a refused build")
        orc = py_oracle.OracleScene(cs, nodes, tris, capi)
        _check_trace(ctx, orc, cs, random_rays(1 << 12, 8, -1.2, 1.2), False)
        _check_trace(ctx, orc, cs, random_rays(1 << 12, 9, -1.2, 1.2), True)
        _check_trace(ctx, orc, cs, edge_rays(), False)

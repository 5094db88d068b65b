"""k_path's traversal iteration and outer loop with the wave-level sets carried as lane masks
 against the oracle.

Bar: bit-exact.  Only how predicates are carried changed: every ray visits the same nodes and leaves in
the same order, pops the same entries and meets the same best, so radiance, weights, the final sampler
state and the per-pixel probe (the ray counts too, in the counting build, whose iteration is the general
source form) equal the oracle's, at path_pop_rounds / path_pop_keep 2 / 4 (the default) and 1 / 64 (every
straggler's pop cut short, so the retry path through AKR_CHILD_POP runs in most iterations).

Renders are forced to k_path, depth 5, SBVH with one-triangle leaves.  The smallest cases that reach each
rewritten path:
  soup     the 20,000-triangle soup of radius 0.1 (test_gpu_pop_defer's "thick"), 48 x 40 px, 4 spp: stacks
           reach the overflow area, so both push forms and both pop forms run in one wave
  partial  the same scene, 37 pixels in one tile: 27 lanes of the only wave are never busy, every mask
           carries idle lanes from the first ballot
  three    3 triangles, 8 x 8 px: the leaves sit in the root's slots, so the first iteration postpones a
           leaf, the pop finds an empty stack and the phase leaves with no lane searching
  gap      2,000 triangles in two slabs at x = -3 and x = +3 and a camera that looks between them: two
           thirds of the pixels' rays cross the root box and enter no slot of the first node (checked on the
           exported BVH2: both children of the root lie outside |x| < 2.5), then pop an empty stack; the
           other pixels walk a slab, where visits that enter no slot are followed by pops that return
           leaves and nodes
  ragged   one render over a ragged, overlapping tile list at depth 0 and at max_depth 9: pixel end, sample
           end and the pending extension ray all pass through the outer loop's flags in one wave
"""
import numpy as np
import pytest

import py_oracle
from akari_amd import capi, scene
from helpers import check_probe, small_soup

pytestmark = pytest.mark.gpu

DEPTH = 5
SETTINGS = [(2, 4), (1, 64)]   # (path_pop_rounds, path_pop_keep)
K_PATH = dict(path=1, path_defer=0, path_spec=0, path_order=0)
RAGGED = [(0, 0, 16, 16), (24, 8, 40, 24), (30, 0, 64, 64), (5, 5, 5, 9)]   # overlapping, clipped, empty


def three_scene(resolution=(8, 8)):
    """A floor triangle, a wall triangle and a one-sided light above them, seen from the front."""
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.6, 0.5, 0.4])), scene.EmissiveMaterial(ct([10.0, 10.0, 10.0]))]
    tris = [([(-2, 0, 2), (2, 0, 2), (0, 0, -2)], (0, 1, 0), 0),
            ([(-2, 0, -1), (2, 0, -1), (0, 3, -1)], (0, 0, 1), 0),
            ([(-1, 2.5, 1), (0, 2.5, -0.9), (1, 2.5, 1)], (0, -1, 0), 1)]
    verts = np.array([p for t in tris for p in t[0]], np.float32)
    mesh = scene.Mesh(verts, np.arange(9, dtype=np.int32).reshape(-1, 3),
                      np.array([list(t[1]) * 3 for t in tris], np.float32),
                      np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (3, 1)),
                      np.array([t[2] for t in tris], np.int32), mats)
    cam = scene.PerspectiveCamera(position=(0.0, 1.2, 4.0), rotation=(0.0, 0.0, 0.0), fov=50.0,
                                  resolution=tuple(resolution))
    return scene.Scene(camera=cam, shapes=[mesh])


GAP_FOV, GAP_DIST, GAP_HALF = 20.0, 20.0, 2.5   # camera at z = 20; no triangle within |x| < 2.55


def gap_scene(resolution=(12, 12)):
    """1,000 triangles of radius 0.15 with centres in [-3.4, -2.7] x [-4, 4] x [-0.5, 0.5], 1,000 in the
    mirrored slab (every tenth of them emissive), and a square image (so the field of view means the same
    along both axes) that spans |x|, |y| < 3.53 at the slabs' depth."""
    rng = np.random.default_rng(7)
    n = 2_000
    c = np.stack([rng.uniform(2.7, 3.4, n) * np.where(np.arange(n) < n // 2, -1.0, 1.0), rng.uniform(-4.0, 4.0, n),
                  rng.uniform(-0.5, 0.5, n)], axis=1)
    verts = (c[:, None, :] + rng.uniform(-0.15, 0.15, (n, 3, 3))).astype(np.float32)
    e1, e2 = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.5, 0.5, 0.5])), scene.EmissiveMaterial(ct([10.0, 10.0, 10.0]), double_sided=True)]
    mesh = scene.Mesh(verts.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(-1, 3),
                      np.repeat(nrm.astype(np.float32), 3, axis=0).reshape(n, 9),
                      np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1)),
                      (np.arange(n) % 10 == 0).astype(np.int32), mats)
    cam = scene.PerspectiveCamera(position=(0.0, 0.0, GAP_DIST), rotation=(0.0, 0.0, 0.0), fov=GAP_FOV,
                                  resolution=tuple(resolution))
    return scene.Scene(camera=cam, shapes=[mesh])


def root_and_children(nodes):
    """(lo, hi) of the exported BVH2's root box and of the root node's two child boxes."""
    box = lambda bxy, bz: (np.array([bxy[0], bxy[2], bz[0]]), np.array([bxy[1], bxy[3], bz[1]]))
    nd = nodes[int(nodes[0]["child"][0])]
    return box(nodes[0]["bxy0"], nodes[0]["bz"][:2]), box(nd["bxy0"], nd["bz"][:2]), box(nd["bxy1"], nd["bz"][2:])


class Case:
    def __init__(self, factory, sc):
        self.ctx = factory(0)
        self.cs = scene.compile_scene(sc)
        scene.upload_scene(self.ctx, self.cs, builder=capi.BUILDER_SBVH, max_leaf_size=1, n_threads=16)
        nodes, tris = self.ctx.accel_export()
        self.nodes = nodes
        self.orc = py_oracle.OracleScene(self.cs, nodes, tris, capi)
        for k, v in K_PATH.items():
            self.ctx.set_option(k, v)
        self.ctx.set_option("pixel_probe", 1)
        self.W, self.H = self.cs.camera.resolution
        self.refs = {}

    def ref(self, spp, depth, tiles):
        """The oracle's render of (spp, depth, tiles): computed once, shared, never written."""
        key = (spp, depth, tuple(tiles))
        if key not in self.refs:
            rad, w, _, probe = self.orc.render(spp, depth, tiles=list(tiles), n_threads=16, probe=True)
            for a in (rad, w, probe):
                a.setflags(write=False)
            self.refs[key] = (rad, w, probe)
        return self.refs[key]

    def check(self, spp, depth, tiles, rounds, keep, count=0):
        ctx, W, H = self.ctx, self.W, self.H
        orad, ow, oprobe = self.ref(spp, depth, tiles)
        what = f"{spp} spp depth {depth} pop_rounds {rounds} pop_keep {keep}{' (counting build)' if count else ''}"
        ctx.set_option("path_pop_rounds", rounds)
        ctx.set_option("path_pop_keep", keep)
        ctx.set_option("count_tests", count)
        ctx.reset_stats()
        try:
            rad, w = ctx.render(spp, depth, list(tiles), W, H)
            assert ctx.render_form()["form"] == "k_path"
            assert np.array_equal(w, ow), f"{what}: weights differ"
            assert np.array_equal(rad, orad), f"{what}: radiance differs (max abs diff {np.abs(rad - orad).max()})"
            n = sum(max(0, min(W, x1) - max(0, x0)) * max(0, min(H, y1) - max(0, y0)) for x0, y0, x1, y1 in tiles)
            counted = check_probe(ctx.pixel_probe(n), oprobe, list(tiles), W, H, what)
            assert counted == bool(count)
            return rad, ctx.path_profile(), ctx.trace_counts()
        finally:
            ctx.set_option("count_tests", 0)


@pytest.fixture(scope="module")
def soup(hip_ctx_factory):
    c = Case(hip_ctx_factory, small_soup(20_000, (48, 40), r=0.1))
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def three(hip_ctx_factory):
    c = Case(hip_ctx_factory, three_scene())
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def gap(hip_ctx_factory):
    c = Case(hip_ctx_factory, gap_scene())
    yield c
    c.ctx.close()


@pytest.mark.parametrize("rounds,keep", SETTINGS)
def test_deep_overlapping_soup(soup, rounds, keep):
    """Whole frame, product and counting build.  The counting build says what the render reached: pushes
    that left LDS (push_slow > push_would_fit), rays in the overflow area, pop rounds beyond the first."""
    tiles = [(0, 0, soup.W, soup.H)]
    rad, _, _ = soup.check(4, DEPTH, tiles, rounds, keep)
    assert rad.mean() > 0
    _, pp, counts = soup.check(4, DEPTH, tiles, rounds, keep, count=1)
    deep_rays = sum(counts["per_mode"][m]["deep_rays"] for m in ("closest", "shadow"))
    print({k: pp[k] for k in ("trav_iters", "pop_iters", "pop_rounds", "pop_lane_rounds", "pop_lanes", "push_iters",
                              "push_slow", "push_would_fit")}, "deep rays", deep_rays)
    assert deep_rays > 0, "no ray reached the overflow stack"
    assert pp["push_slow"] > pp["push_would_fit"] > 0     # both push forms
    assert pp["pop_lane_rounds"] > 0 and pp["pop_lanes"] > 0
    if rounds == 1:
        assert pp["pop_rounds"] == pp["pop_iters"] > 0    # one round per iteration: every straggler retries


@pytest.mark.parametrize("rounds,keep", SETTINGS)
def test_partial_wave(soup, rounds, keep):
    """37 pixels in one tile: one wave, 27 of its lanes never busy."""
    tiles = [(5, 3, 42, 4)]
    rad, _, _ = soup.check(4, DEPTH, tiles, rounds, keep)
    assert np.count_nonzero(rad.sum(axis=2)) > 0
    soup.check(4, DEPTH, tiles, rounds, keep, count=1)


@pytest.mark.parametrize("rounds,keep", SETTINGS)
def test_leaves_in_the_roots_slots(three, rounds, keep):
    """Three triangles: every slot of the only node is a leaf or empty."""
    tiles = [(0, 0, three.W, three.H)]
    rad, _, _ = three.check(4, DEPTH, tiles, rounds, keep)
    assert rad.mean() > 0
    _, pp, counts = three.check(4, DEPTH, tiles, rounds, keep, count=1)
    cl, sh = counts["per_mode"]["closest"], counts["per_mode"]["shadow"]
    print("visits", cl["visits"], sh["visits"], "rays", cl["rays"], sh["rays"], "pop_iters", pp["pop_iters"])
    assert cl["visits"] <= cl["rays"] and sh["visits"] <= sh["rays"]   # no node below the root
    assert pp["pop_iters"] > 0


@pytest.mark.parametrize("rounds,keep", SETTINGS)
def test_no_slot_entered(gap, rounds, keep):
    """Most camera rays cross the root box between the two slabs and enter no slot of the first node."""
    (rlo, rhi), (alo, ahi), (blo, bhi) = root_and_children(gap.nodes)
    # the tree: the root box spans the gap, both children of the root lie beside it (the first wide node's
    # slots are these children or their children, quantized outward by less than 1/255 of the node's extent)
    assert rlo[0] < -GAP_HALF and rhi[0] > GAP_HALF and rlo[1] < -3.9 and rhi[1] > 3.9
    assert min(ahi[0], bhi[0]) < -GAP_HALF and max(alo[0], blo[0]) > GAP_HALF
    # the pixels: a pixel's rays pass the slabs' depth inside its footprint there
    half = GAP_DIST * np.tan(np.radians(GAP_FOV / 2))
    xs = (np.arange(gap.W) + 0.5) / gap.W * 2 * half - half
    in_gap = np.abs(xs) + half / gap.W + 0.05 < GAP_HALF       # the whole footprint, with a margin
    assert in_gap.mean() >= 0.6 and half < 3.9
    tiles = [(0, 0, gap.W, gap.H)]
    gap.check(4, DEPTH, tiles, rounds, keep)
    _, oprobe = gap.ref(4, DEPTH, tiles)[1:]
    assert np.all(oprobe["closest_rays"][:, in_gap] == 4) and np.all(oprobe["shadow_rays"][:, in_gap] == 0)
    assert oprobe["closest_rays"][:, ~in_gap].max() > 4       # the other columns hit a slab and bounce
    _, pp, counts = gap.check(4, DEPTH, tiles, rounds, keep, count=1)
    cl = counts["per_mode"]["closest"]
    print("closest rays", cl["rays"], "visits", cl["visits"], "leaf tests", cl["leaf_tests"], "pop_iters", pp["pop_iters"])
    # every ray of a gap pixel is one closest-hit ray with exactly one visit, the root's, and no leaf test
    n_gap = 4 * gap.H * int(in_gap.sum())
    assert cl["rays"] >= n_gap + 4 * gap.H * int((~in_gap).sum()) and cl["visits"] >= n_gap
    assert pp["pop_iters"] > 0


@pytest.mark.parametrize("depth", [0, 9])
def test_overlapping_tile_list(soup, depth):
    """A ragged, overlapping, partly empty tile list in one render; depth 0 ends every sample at its camera
    ray, depth 9 keeps extension rays pending behind shadow rays for nine bounces."""
    for rounds, keep in SETTINGS:
        soup.check(3, depth, RAGGED, rounds, keep)
    soup.check(3, depth, RAGGED, 2, 4, count=1)

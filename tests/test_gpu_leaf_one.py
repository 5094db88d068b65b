"""k_path's leaf phase for one-triangle leaves against the oracle.

Bar: bit-exact.  A device leaf reference says whether its leaf holds one triangle.  On a tree whose leaves are
at least 97 % of that kind the host launches the kernel with the one-triangle leaf phase: a wave none of whose
leaf holders lacks the flag takes a straight-line block (five loads, the exact box, Moller-Trumbore as values
and masks), a wave with any larger leaf among its holders takes the general form for every holder.  On any
other tree the kernel with the general form alone runs.  Every ray meets the same boxes and triangles in the
same order with the same operations, so radiance, weights, the final sampler state and, in the counting build
(which keeps the general form), the per-pixel ray counts equal the oracle's.

Renders are forced to k_path, at most 32 x 32 px and 4 spp:
  flagged   the 20,000-triangle soup of radius 0.1 with its light quad, and the Cornell box, each built with
            max_leaf_size 1 by the SBVH and by the LBVH builder: every leaf holds one triangle (checked on the
            exported BVH2), so every leaf phase of the product build is the straight-line block.  Depth 0, 5
            and 9, a ragged overlapping tile list, a wave with idle lanes; the soup's stacks reach the
            overflow area (checked in the counting build)
  mixed     a small soup in which every other triangle has two or three coincident copies, max_leaf_size 4:
            leaves of one triangle beside leaves of 2-4 (each kind at least a quarter of the leaves, checked on
            the exported BVH2), so waves hold both kinds; the copies tie exactly in t
            (37 % of the leaves hold one triangle, so the general kernel runs, with flagged references)
  mostly    the same soup with copies of every 50th triangle only, binned SAH builder: 98 % one-triangle leaves,
            so the kernel with the block runs and about a third of its leaf phases meet a larger leaf
  needles   flagged leaves of near-degenerate triangles: needles, zero-area triangles (det = 0, 1 / det
            infinite) and triangles in planes through the camera position (det on both sides of +-1e-6)
"""
import numpy as np
import pytest

import py_oracle
from akari_amd import capi, scene
from helpers import check_probe, cornell, small_soup

pytestmark = pytest.mark.gpu

K_PATH = dict(path=1, path_defer=0, path_spec=0, path_order=0)
RAGGED = [(0, 0, 16, 16), (12, 8, 30, 24), (20, 0, 64, 64), (5, 5, 5, 9)]   # overlapping, clipped, empty
PARTIAL = [(3, 2, 32, 3), (0, 7, 8, 8)]                                     # 29 + 8 pixels: one wave, 27 idle lanes


def leaf_counts(nodes):
    """Triangles per leaf over the exported BVH2's leaf references."""
    ch = nodes["child"].reshape(-1).astype(np.int64)
    refs = ch[(ch != 0xFFFFFFFF) & ((ch & 0x80000000) != 0)]
    return (refs & 7) + 1


def mesh_scene(verts, mats, mat_ids, cam):
    verts = np.asarray(verts, np.float32).reshape(-1, 3, 3)
    n = len(verts)
    nrm = np.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0])
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(length > 1e-20, nrm / np.maximum(length, 1e-20), np.array([0.0, 1.0, 0.0]))
    mesh = scene.Mesh(verts.reshape(-1, 3), np.arange(3 * n, dtype=np.int32).reshape(-1, 3),
                      np.repeat(nrm.astype(np.float32), 3, axis=0).reshape(n, 9),
                      np.tile(np.array([0, 0, 1, 0, 0, 1], np.float32), (n, 1)), np.asarray(mat_ids, np.int32), mats)
    return scene.Scene(camera=cam, shapes=[mesh])


LIGHT_QUAD = [[(-1, 1.5, -1), (1, 1.5, -1), (1, 1.5, 1)], [(-1, 1.5, -1), (1, 1.5, 1), (-1, 1.5, 1)]]   # faces down


def mixed_scene(resolution=(24, 24), n=600, seed=11, every=2):
    """n triangles of radius 0.12 with centres in [-1, 1]^3; every `every`-th one is followed by one or two
    exact copies of itself; and a light quad above."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, (n, 1, 3)) + rng.uniform(-0.12, 0.12, (n, 3, 3))
    tris = []
    for i, t in enumerate(base):
        tris += [t] * (1 if i % every != every - 1 else 2 + (i // every) % 2)
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.6, 0.55, 0.5])), scene.EmissiveMaterial(ct([10.0, 10.0, 10.0]))]
    verts = np.concatenate([np.array(tris), np.array(LIGHT_QUAD, np.float64)])
    cam = scene.PerspectiveCamera(position=(0.0, 0.0, 4.0), rotation=(0.0, 0.0, 0.0), fov=40.0, resolution=tuple(resolution))
    return mesh_scene(verts, mats, [0] * len(tris) + [1, 1], cam)


CAM = np.array([0.0, 0.5, 4.0])


def needle_scene(resolution=(32, 32), seed=5):
    """A floor, a back wall and a light; in front of the wall 60 needles (two long edges 1e-5 to 1e-3 apart), 20
    zero-area triangles (two equal vertices, or three on a line) and 60 triangles whose plane contains the
    camera position, which every camera ray therefore meets edge-on."""
    rng = np.random.default_rng(seed)
    tris = [[(-3, -1, 3), (3, -1, 3), (3, -1, -3)], [(-3, -1, 3), (3, -1, -3), (-3, -1, -3)],
            [(-3, -1, -2), (3, -1, -2), (3, 3, -2)], [(-3, -1, -2), (3, 3, -2), (-3, 3, -2)]]
    for k in range(60):      # needles
        a = rng.uniform(-1.2, 1.2, 3) * [1, 0.8, 0.5] + [0, 0.5, 0]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        side = np.cross(d, rng.normal(size=3))
        side /= np.linalg.norm(side)
        tris.append([a, a + d * rng.uniform(0.5, 1.5), a + d * 0.5 + side * 10.0 ** rng.uniform(-5, -3)])
    for k in range(20):      # no area at all
        a, b = rng.uniform(-1, 1, 3) + [0, 0.5, 0], rng.uniform(-1, 1, 3) + [0, 0.5, 0]
        tris.append([a, b, b] if k % 2 else [a, b, a + 0.25 * (b - a)])
    for k in range(60):      # edge-on: the camera position and two points in front of it span the plane
        p, q = rng.uniform(-1.5, 1.5, 3) * [1, 0.7, 0.3] + [0, 0.5, 0], rng.uniform(-1.5, 1.5, 3) * [1, 0.7, 0.3] + [0, 0.5, 0]
        a, b, c = CAM + 0.6 * (p - CAM), CAM + 1.0 * (p - CAM), CAM + rng.uniform(0.7, 0.9) * (q - CAM)
        tris.append([a, b, c])
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.6, 0.6, 0.6])), scene.EmissiveMaterial(ct([10.0, 10.0, 10.0]))]
    light = (np.array(LIGHT_QUAD, np.float64) * [0.5, 1, 0.5] + [0, 1.0, 0]).tolist()
    verts = np.array([np.asarray(t, np.float64) for t in tris] + [np.asarray(t) for t in light])
    cam = scene.PerspectiveCamera(position=tuple(CAM), rotation=(0.0, 0.0, 0.0), fov=45.0, resolution=tuple(resolution))
    return mesh_scene(verts, mats, [0] * len(tris) + [1, 1], cam)


class Case:
    def __init__(self, factory, sc, builder, max_leaf):
        self.ctx = factory(0)
        self.cs = scene.compile_scene(sc)
        scene.upload_scene(self.ctx, self.cs, builder=builder, max_leaf_size=max_leaf, n_threads=16)
        self.nodes, tris = self.ctx.accel_export()
        self.tris = tris
        self.orc = py_oracle.OracleScene(self.cs, self.nodes, tris, capi)
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

    def check(self, spp, depth, tiles, count=0):
        ctx, W, H = self.ctx, self.W, self.H
        orad, ow, oprobe = self.ref(spp, depth, tiles)
        what = f"{spp} spp depth {depth}{' (counting build)' if count else ''}"
        ctx.set_option("count_tests", count)
        ctx.reset_stats()
        try:
            rad, w = ctx.render(spp, depth, list(tiles), W, H)
            assert ctx.render_form()["form"] == "k_path"
            assert np.array_equal(w, ow), f"{what}: weights differ"
            assert np.array_equal(rad, orad), f"{what}: radiance differs (max abs diff {np.abs(rad - orad).max()})"
            n = sum(max(0, min(W, x1) - max(0, x0)) * max(0, min(H, y1) - max(0, y0)) for x0, y0, x1, y1 in tiles)
            assert check_probe(ctx.pixel_probe(n), oprobe, list(tiles), W, H, what) == bool(count)
            return rad, ctx.trace_counts()
        finally:
            ctx.set_option("count_tests", 0)

    def both(self, spp, depth, tiles):
        """Product build, then counting build; the product build's film and the counting build's tallies."""
        rad, _ = self.check(spp, depth, tiles)
        return rad, self.check(spp, depth, tiles, count=1)[1]


BUILDERS = {"sbvh": capi.BUILDER_SBVH, "lbvh": capi.BUILDER_LBVH}
ONE_SHARE = 0.97       # csrc/leaf_layout.h leaf_one_pays: from this share of one-triangle leaves the block's kernel runs


@pytest.fixture(scope="module", params=["soup-sbvh", "soup-lbvh", "cornell-sbvh", "cornell-lbvh"])
def flagged(request, hip_ctx_factory):
    name, builder = request.param.split("-")
    sc = small_soup(20_000, (32, 32), r=0.1) if name == "soup" else cornell((32, 32))
    c = Case(hip_ctx_factory, sc, BUILDERS[builder], 1)
    c.name = name
    assert np.all(leaf_counts(c.nodes) == 1)      # every device leaf reference carries the flag
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def mixed(hip_ctx_factory):
    c = Case(hip_ctx_factory, mixed_scene(), capi.BUILDER_SBVH, 4)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def mostly(hip_ctx_factory):
    c = Case(hip_ctx_factory, mixed_scene(every=50), capi.BUILDER_SAH, 4)
    yield c
    c.ctx.close()


@pytest.fixture(scope="module")
def needles(hip_ctx_factory):
    c = Case(hip_ctx_factory, needle_scene(), capi.BUILDER_SBVH, 1)
    yield c
    c.ctx.close()


@pytest.mark.parametrize("depth", [0, 5, 9])
def test_every_leaf_flagged(flagged, depth):
    """Whole frame.  The soup's counting build says that stacks reached the overflow area."""
    rad, counts = flagged.both(4, depth, [(0, 0, flagged.W, flagged.H)])
    assert rad.mean() > 0
    cl, sh = counts["per_mode"]["closest"], counts["per_mode"]["shadow"]
    print(flagged.name, "depth", depth, "leaf tests", cl["leaf_tests"], sh["leaf_tests"], "tri tests", cl["tri_tests"],
          sh["tri_tests"], "deep rays", cl["deep_rays"], sh["deep_rays"])
    assert cl["tri_tests"] > 0 and cl["tri_tests"] <= cl["leaf_tests"]       # at most one triangle per leaf test
    if depth:
        assert sh["rays"] > 0
    if flagged.name == "soup" and depth:
        assert cl["deep_rays"] + sh["deep_rays"] > 0, "no ray reached the overflow stack"


def test_flagged_ragged_tile_list(flagged):
    flagged.both(3, 5, RAGGED)


def test_flagged_wave_with_idle_lanes(flagged):
    """37 pixels: the only wave holds 27 lanes that are never busy."""
    rad, _ = flagged.both(4, 5, PARTIAL)
    assert np.count_nonzero(rad.sum(axis=2)) > 0


def test_mixed_waves(mixed):
    """Leaves of one triangle beside leaves of two to four in the same waves, and exact ties in t among the
    coincident copies, which the strict t < best resolves by the order of the records."""
    n = leaf_counts(mixed.nodes)
    print("leaves by count", np.bincount(n))
    assert n.max() <= 4 and ONE_SHARE > (n == 1).mean() >= 0.25 and (n > 1).mean() >= 0.25
    # the copies are there: fewer distinct triangle records than records
    v = np.concatenate([mixed.tris[k] for k in ("v0", "e1", "e2")], axis=1)
    assert len(np.unique(v, axis=0)) < 0.7 * len(v)
    for depth, tiles in ((5, [(0, 0, mixed.W, mixed.H)]), (9, RAGGED), (5, PARTIAL)):
        rad, counts = mixed.both(4, depth, tiles)
        cl = counts["per_mode"]["closest"]
        assert rad.mean() > 0 and cl["tri_tests"] > cl["leaf_tests"]      # leaves of several triangles met
    assert cl["tri_tests"] > 0


def test_mostly_flagged_mixed_waves(mostly):
    """The kernel with the block on a tree that also has larger leaves: a wave with one of them among its
    holders takes the general form for all, the other waves the block; the copies tie exactly in t."""
    n = leaf_counts(mostly.nodes)
    print("leaves by count", np.bincount(n))
    assert ONE_SHARE <= (n == 1).mean() < 0.99 and (n > 1).sum() >= 10
    for depth, tiles in ((5, [(0, 0, mostly.W, mostly.H)]), (9, RAGGED), (5, PARTIAL)):
        rad, counts = mostly.both(4, depth, tiles)
        assert rad.mean() > 0


def test_near_degenerate_triangles(needles):
    """Flagged leaves whose triangle has det inside +-1e-6, det = 0 (1 / det infinite, u and v NaN or infinite)
    or a needle's shape: the film is finite and the oracle's."""
    assert np.all(leaf_counts(needles.nodes) == 1)
    # the input: det = e1 . (d x e2) in f32 for rays through the pixel centres
    half = np.tan(np.radians(45.0 / 2))
    ys, xs = np.mgrid[0:needles.H, 0:needles.W]
    d = np.stack([((xs + 0.5) / needles.W * 2 - 1) * half, (1 - (ys + 0.5) / needles.H * 2) * half,
                  -np.ones(xs.shape)], -1).reshape(-1, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    h = np.cross(d[:, None, :], needles.tris["e2"][None, :, :]).astype(np.float32)
    det = (h * needles.tris["e1"][None]).sum(-1, dtype=np.float32)
    small, zero = (np.abs(det) < 1e-6) & (det != 0), det == 0
    print("ray-triangle pairs", det.size, "det inside +-1e-6", np.count_nonzero(small), "det = 0", np.count_nonzero(zero))
    assert np.count_nonzero(small) > 1000 and np.count_nonzero(zero) > 100
    assert np.any(small & (det > 0)) and np.any(small & (det < 0))
    for depth in (0, 5):
        rad, _ = needles.both(4, depth, [(0, 0, needles.W, needles.H)])
        assert np.all(np.isfinite(rad)) and (rad.mean() > 0 or depth == 0)    # (the light lies outside the view)
    orad = needles.ref(4, 5, ((0, 0, needles.W, needles.H),))[0]
    assert np.all(np.isfinite(orad))

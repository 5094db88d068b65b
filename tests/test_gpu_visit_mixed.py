"""k_path's trimmed wide-node visit (the pushed pairs as two dwords of one LDS instruction,
order and push without compares, tmin and the exit bound not re-canonicalised per visit) against the oracle
and against the counting build, which keeps the earlier visit.  (The file keeps the name its issue gave it;
the mixed-precision slot bounds it was named for were measured and left out, EXPERIMENTS.md §15.)

Bar: bit-exact.  Every ray visits the same nodes and leaves in the same order and pushes the same entries, so
radiance, weights and the per-pixel probe (final sampler state; the ray counts too in the counting build) are
the oracle's, and the product build's film is the counting build's.  Films are 96 x 54, renders forced to the
persistent k_path form, SBVH trees: max_leaf_size 1 makes one-triangle leaves (k_path / k_path_env),
max_leaf_size 4 with cheap triangle tests a tree below leaf_layout.h's 97 % rule (k_path_general /
k_path_env_general), checked on the exported BVH2.

Not here: direction components of +-2^-62 .. 2^-64 cannot be asked of a camera, whose rays are the pixel
grid's; those directions reach the visit's untrimmed instantiation in test_gpu_trace_limits.py, and the
trimmed visit's slot arithmetic is that instantiation's.  The oracle has no environment light, so the environment
renders are compared with the counting build and with the wavefront form (k_trace's untrimmed visit).
"""
import numpy as np
import pytest

import py_oracle
from akari_amd import capi, scene
from helpers import check_probe, scaled_soup, small_soup
from test_gpu_leaf_one import LIGHT_QUAD, leaf_counts, mesh_scene

pytestmark = pytest.mark.gpu

W, H = 96, 54
FRAME = [(0, 0, W, H)]
K_PATH = dict(path=1, path_defer=0, path_spec=0, path_order=0)
BUILD = dict(builder=capi.BUILDER_SBVH, n_threads=16)
LEAVES = {1: dict(max_leaf_size=1), 4: dict(max_leaf_size=4, traversal_cost=4.0, intersect_cost=0.25)}


class View:
    """A context holding one scene, forced to k_path, with the oracle of its exported BVH2."""

    def __init__(self, factory, sc, max_leaf, bvh=None, **options):
        self.ctx = factory(0)
        self.cs = scene.compile_scene(sc)
        if bvh is None:
            scene.upload_scene(self.ctx, self.cs, **LEAVES[max_leaf], **BUILD)
        else:
            scene.upload_scene(self.ctx, self.cs, bvh=bvh, n_threads=16)
        self.nodes, self.tris = self.ctx.accel_export()
        counts = leaf_counts(self.nodes)
        if max_leaf == 1:
            assert np.all(counts == 1)
        else:
            assert counts.max() > 1 and np.mean(counts == 1) < 0.97, np.bincount(counts)
        self.orc = None if self.cs.environment is not None else py_oracle.OracleScene(self.cs, self.nodes, self.tris, capi)
        for k, v in {**K_PATH, **options, "pixel_probe": 1}.items():
            self.ctx.set_option(k, v)

    def render(self, spp, depth, tiles, count):
        ctx = self.ctx
        ctx.set_option("count_tests", count)
        ctx.reset_stats()
        try:
            rad, w = ctx.render(spp, depth, list(tiles), W, H)
            assert ctx.render_form()["form"] == "k_path", ctx.render_form()
            n = sum(max(0, min(W, x1) - max(0, x0)) * max(0, min(H, y1) - max(0, y0)) for x0, y0, x1, y1 in tiles)
            return rad, w, ctx.pixel_probe(n), ctx.path_profile(), ctx.trace_counts()
        finally:
            ctx.set_option("count_tests", 0)

    def check(self, spp, depth, tiles=FRAME, what="", nan_ok=False):
        """Product build == counting build (the earlier visit) == oracle.  Returns the film and the counting
        build's profile and counters.  nan_ok: a NaN equals a NaN in the same place."""
        same = lambda a, b: np.array_equal(a, b, equal_nan=nan_ok)
        rad, w, probe, _, _ = self.render(spp, depth, tiles, 0)
        crad, cw, cprobe, pp, counts = self.render(spp, depth, tiles, 1)
        assert np.array_equal(w, cw), f"{what}: weights differ from the counting build's"
        assert same(rad, crad), f"{what}: the film differs from the counting build's (max {np.abs(rad - crad).max()})"
        assert np.array_equal(probe["seed"], cprobe["seed"]), f"{what}: sampler states differ from the counting build's"
        if self.orc is not None:
            orad, ow, _, oprobe = self.orc.render(spp, depth, tiles=list(tiles), n_threads=16, probe=True)
            assert np.array_equal(w, ow), f"{what}: weights differ from the oracle's"
            assert same(rad, orad), f"{what}: the film differs from the oracle's (max {np.abs(rad - orad).max()})"
            assert not check_probe(probe, oprobe, list(tiles), W, H, what)
            assert check_probe(cprobe, oprobe, list(tiles), W, H, what + " (counting build)")
        self.weight = w
        return rad, pp, counts


@pytest.fixture(scope="module", params=[1, 4], ids=["k_path", "k_path_general"])
def soup(request, hip_ctx_factory):
    v = View(hip_ctx_factory, small_soup(20_000, (W, H)), request.param)
    yield v
    v.ctx.close()


@pytest.mark.parametrize("depth", [0, 5, 9])
def test_soup_at_depth(soup, depth):
    """The 20,000-triangle soup in both product kernels: camera rays alone, the default depth, long paths."""
    rad, _, counts = soup.check(2, depth, what=f"depth {depth}")
    assert counts["per_mode"]["closest"]["visits"] > 0
    assert depth == 0 or rad.mean() > 0        # (no camera ray sees the light quad, which faces down)


def _sky(n=8):
    """A small octahedral map: a smooth ramp with one bright texel."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    img = np.stack([0.2 + x / n, 0.3 + y / n, 0.5 + 0.0 * x], axis=2).astype(np.float32)
    img[1, 2] = (20.0, 18.0, 15.0)
    return scene.EnvironmentLight(image=img)


@pytest.mark.parametrize("max_leaf", [1, 4], ids=["k_path_env", "k_path_env_general"])
@pytest.mark.parametrize("depth", [0, 5, 9])
def test_soup_under_a_sky(hip_ctx_factory, max_leaf, depth):
    """The same soup under option env_path 1 with a small sky: the environment builds of both kernels."""
    sc = small_soup(20_000, (W, H))
    sc.environment = _sky()
    v = View(hip_ctx_factory, sc, max_leaf, env_path=1)
    try:
        rad, _, _ = v.check(2, depth, what=f"sky, depth {depth}")
        assert rad.mean() > 0                      # the sky is seen at every depth
        v.ctx.set_option("path", 0)
        wrad, ww = v.ctx.render(2, depth, FRAME, W, H)
        assert v.ctx.render_form()["form"] == "wavefront"
        assert np.array_equal(ww, v.weight) and np.array_equal(rad, wrad)
    finally:
        v.ctx.close()


@pytest.mark.parametrize("k", [0, 20, 38, 39])
def test_scaled_soup(hip_ctx_factory, k):
    """The soup of large triangles and its camera scaled by 2^k, up to the last scale the view's 2^40 gate
    admits (frame origins up to 1.2 * 2^k).  The shading is not made for these scales: the oracle's film is
    black from 2^20 on and mostly NaN at 2^39, where paths end after one bounce.  What pins the traversal
    there is the per-pixel probe: the final sampler state in the product build (it depends on every hit or
    miss that lengthened or ended a path) and the counting build's rays per pixel, both against the
    oracle's; the films are compared all the same, a NaN equal to a NaN in its place."""
    sc = scaled_soup(k, (W, H))
    sc.camera = scene.PerspectiveCamera(position=(0.0, 0.0, 4.0 * 2.0 ** k), rotation=(0.0, 0.0, 0.0), fov=40.0,
                                        resolution=(W, H))
    v = View(hip_ctx_factory, sc, 1)
    try:
        rad, _, counts = v.check(2, 5, what=f"scale 2^{k}", nan_ok=True)
        assert k > 0 or (np.isfinite(rad).all() and rad.mean() > 0)
        assert counts["per_mode"]["closest"]["visits"] > W * H
        assert counts["per_mode"]["closest"]["rays"] >= 3 * W * H      # paths go on past their camera rays
    finally:
        v.ctx.close()


def bytes_scene(camera):
    """9,000 triangles with centres in [-1, 1]^3 and radii from 0.002 to 0.3 (so slot boxes start and end
    anywhere in their node's grid), and the light quad."""
    rng = np.random.default_rng(19)
    n = 9000
    r = 0.002 * 150.0 ** rng.random((n, 1, 1))
    tris = rng.uniform(-1.0, 1.0, (n, 1, 3)) + r * rng.uniform(-1.0, 1.0, (n, 3, 3))
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.6, 0.55, 0.5])), scene.EmissiveMaterial(ct([10.0, 10.0, 10.0]), double_sided=True)]
    return mesh_scene(np.concatenate([tris, np.array(LIGHT_QUAD, np.float64)]), mats, [0] * n + [1, 1], camera)


def _camera(rx, ry):
    return scene.PerspectiveCamera(position=(0.0, 0.0, 0.0), rotation=(rx, ry, 0.0), fov=60.0, resolution=(W, H))


def test_slot_bytes_at_the_ends_of_their_range(hip_ctx_factory):
    """Slot bytes 0, 1, 254 and 255 in every byte lane and on every axis (read from the wide view of the
    tree the device holds), seen from the middle of the scene along the eight octants' diagonals."""
    cs = scene.compile_scene(bytes_scene(_camera(0.0, 0.0)))
    nodes, tris, _, (wn, _, _) = capi.build_bvh_host(cs.vertices, cs.indices, max_leaf_size=1, wide=True, **BUILD)
    live = wn["child"] != 0xFFFFFFFF                                  # [node, slot]
    for axis in range(3):
        for lane in range(4):
            lo = (wn["q"][:, 2 * axis] >> (8 * lane)) & 0xFF
            hi = (wn["q"][:, 2 * axis + 1] >> (8 * lane)) & 0xFF
            seen = set(lo[live[:, lane]].tolist()) | set(hi[live[:, lane]].tolist())
            assert {0, 1, 254, 255} <= seen, (axis, lane, sorted(seen)[:3], sorted(seen)[-3:])
    means = []
    for rx in (35.0, -35.0):
        for ry in (45.0, 135.0, 225.0, 315.0):
            v = View(hip_ctx_factory, bytes_scene(_camera(rx, ry)), 1, bvh=(nodes, tris))
            try:
                assert np.array_equal(v.nodes, nodes)                  # the device walks the tree read above
                rad, _, _ = v.check(1, 5, what=f"camera rotation ({rx}, {ry})")
                means.append(float(rad.mean()))
            finally:
                v.ctx.close()
    assert len(set(means)) == 8 and min(means) > 0                    # eight different views, none empty


@pytest.fixture(scope="module")
def thick(hip_ctx_factory):
    v = View(hip_ctx_factory, small_soup(20_000, (W, H), r=0.1), 1)
    yield v
    v.ctx.close()


def test_deep_overlapping_soup_pushes(thick):
    """Triangles of radius 0.1: stacks reach the overflow area, so the straight-line push (pairs, `dead`
    word) and the pushes that leave LDS run in the same waves."""
    rad, pp, counts = thick.check(2, 5, what="thick soup")
    deep = sum(counts["per_mode"][m]["deep_rays"] for m in ("closest", "shadow"))
    assert rad.mean() > 0 and deep > 0, "no ray reached the overflow stack"
    assert pp["push_slow"] > pp["push_would_fit"] > 0


def test_wave_with_idle_lanes(thick):
    """37 pixels in one tile: one wave, 27 of its lanes never busy."""
    rad, _, _ = thick.check(2, 5, tiles=[(5, 3, 42, 4)], what="partial wave")
    assert np.count_nonzero(rad.sum(axis=2)) > 0

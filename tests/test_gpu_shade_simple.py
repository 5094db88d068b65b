"""The persistent path kernels' two shading builds against the oracle.

Bar: bit-exact.  On a scene whose committed tables hold constant Diffuse / Emissive only (csrc/shade_simple.h)
the product builds of k_path, k_path_spec and k_path_defer run the simple shading build: the general one with
the texcoord fetch, the image lookups, the Mix selection and the Glossy closure folded away.  It runs the same
operations in the same order for everything that is left, so radiance, weights, the final sampler states
and, in the counting build (which keeps the general shading, and so cross-checks the two), the per-pixel ray
counts equal the oracle's.  On every other scene, and in the counting build, the general build runs.
render_info()["shading"] says which one a render ran.

Renders are at most 96 x 64 px and 3 spp:
  simple     the Cornell box on a ragged 96 x 64 tile list and the 20,000-triangle soup with its emitter: depth
             0, 1 and 5; forced to k_path, k_path_spec and k_path_defer; tables in LDS and not; product build
             (reports "simple") and counting build (reports "general")
  emitters   a front-only and a double-sided emitter seen from behind and a triangle without a material, at
             depth 0 and 5
  complex    scenes one step from simple (two Diffuse under a Mix, one Glossy, an image on a diffuse colour, an
             image on the light's emission alone), forced to each persistent form: each reports "general"
  sequence   one context: simple scene; complex scene; the simple scene again and a continued render of it.
             The reported build follows the committed scene (a stale flag is how this dispatch goes wrong)
"""
import numpy as np
import pytest

import py_oracle
from akari_amd import capi, scene
from helpers import check_probe, cornell, small_soup, tri_scene

pytestmark = pytest.mark.gpu

FORMS = {
    "k_path": dict(path=1, path_defer=0, path_spec=0),
    "k_path_spec": dict(path=1, path_defer=0, path_spec=1),
    "k_path_defer": dict(path=1, path_defer=1, path_spec=0),
}
RAGGED = [(0, 0, 16, 16), (12, 8, 30, 24), (40, 3, 96, 64), (5, 5, 5, 9), (90, 60, 120, 70)]   # overlapping, clipped, empty
SPP = 3


def n_slots(tiles, W, H):
    return sum(max(0, min(W, x1) - max(0, x0)) * max(0, min(H, y1) - max(0, y0)) for x0, y0, x1, y1 in tiles)


class Case:
    """A context holding one scene and the oracle over the context's own tree."""

    def __init__(self, ctx, sc):
        self.ctx = ctx
        self.cs = scene.compile_scene(sc)
        scene.upload_scene(ctx, self.cs, n_threads=16)
        nodes, tris = ctx.accel_export()
        self.orc = py_oracle.OracleScene(self.cs, nodes, tris, capi)
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("path_order", 0)
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

    def compare(self, rad, w, spp, depth, tiles, what, count=False):
        orad, ow, oprobe = self.ref(spp, depth, tiles)
        assert np.array_equal(w, ow), f"{what}: weights differ"
        assert np.array_equal(rad, orad), f"{what}: radiance differs (max abs diff {np.abs(rad - orad).max()})"
        probe = self.ctx.pixel_probe(n_slots(tiles, self.W, self.H))
        rays = check_probe(probe, oprobe, list(tiles), self.W, self.H, what)
        # a persistent form counts rays in its counting build alone (count None: not a persistent form)
        assert count is None or rays == bool(count), what

    def check(self, form, depth, tiles, shading, tab=1, count=0, spp=SPP):
        ctx = self.ctx
        what = f"{form} tab {tab} depth {depth}{' (counting build)' if count else ''}"
        for k, v in FORMS[form].items():
            ctx.set_option(k, v)
        ctx.set_option("path_tab", tab)
        ctx.set_option("count_tests", count)
        try:
            rad, w = ctx.render(spp, depth, list(tiles), self.W, self.H)
            assert ctx.render_form()["form"] == form, what
            # the counting build shades with the general build on every scene
            assert ctx.render_info()["shading"] == ("general" if count else shading), what
            self.compare(rad, w, spp, depth, tiles, what, count)
            return rad
        finally:
            ctx.set_option("count_tests", 0)
            ctx.set_option("path_tab", 1)


@pytest.fixture(scope="module", params=["cornell", "soup"])
def simple(request, hip_ctx_factory):
    sc = cornell((96, 64)) if request.param == "cornell" else small_soup(20_000, (32, 32), r=0.1)
    ctx = hip_ctx_factory(0)
    c = Case(ctx, sc)
    c.tiles = RAGGED if request.param == "cornell" else [(0, 0, 32, 32)]
    yield c
    ctx.close()


@pytest.mark.parametrize("depth", [0, 1, 5])
def test_simple_scenes_every_form(simple, depth):
    for form in FORMS:
        for tab in (0, 1):
            rad = simple.check(form, depth, simple.tiles, "simple", tab=tab)
            simple.check(form, depth, simple.tiles, "simple", tab=tab, count=1)
    assert depth == 0 or rad.mean() > 0      # (depth 0 adds a directly seen emitter's front alone: the box shows none)


def emitter_scene(resolution=(32, 32)):
    """Seen from z = 4: a grey floor and back wall; a front-only emitter and a double-sided one, both turned
    away from the camera (their normals point to -z), each also a light; a triangle without a material in
    front of the wall; and a front-only emitter above the view, facing down, which lights the rest."""
    ct = scene.ConstantTexture
    mats = [scene.DiffuseMaterial(ct([0.6, 0.55, 0.5])), scene.EmissiveMaterial(ct([9.0, 6.0, 3.0]), double_sided=False),
            scene.EmissiveMaterial(ct([2.0, 5.0, 8.0]), double_sided=True), scene.EmissiveMaterial(ct([12.0, 12.0, 12.0]))]
    tris = [[(-3, -1, 3), (3, -1, 3), (3, -1, -3)], [(-3, -1, 3), (3, -1, -3), (-3, -1, -3)],          # floor
            [(-3, -1, -2), (3, -1, -2), (3, 3, -2)], [(-3, -1, -2), (3, 3, -2), (-3, 3, -2)],          # back wall
            [(-1.2, -0.5, 0), (-0.2, 0.8, 0), (-0.2, -0.5, 0)],      # front-only, normal -z: dark from the camera
            [(0.2, -0.5, 0), (1.2, 0.8, 0), (1.2, -0.5, 0)],         # double-sided, normal -z: seen
            [(-0.6, 0.9, -1), (0.6, 0.9, -1), (0.0, 1.6, -1)],       # no material: the path ends there
            [(0.5, 3.0, 1.0), (-0.5, 3.0, 1.0), (0.0, 3.0, 0.0)]]    # above the view: faces down and lights the scene
    cam = scene.PerspectiveCamera(position=(0.0, 0.5, 4.0), rotation=(0.0, 0.0, 0.0), fov=45.0, resolution=tuple(resolution))
    return tri_scene(tris, mats, [0, 0, 0, 0, 1, 2, -1, 3], cam)


def test_emitters_from_behind_and_a_null_material(hip_ctx_factory):
    with hip_ctx_factory(0) as ctx:
        c = Case(ctx, emitter_scene())
        # the input: the three triangles' normals point away from the camera; both emitters are lights
        v = np.asarray(c.cs.meshes[0].vertices, np.float64).reshape(-1, 3, 3)
        assert np.all(np.cross(v[4:6, 1] - v[4:6, 0], v[4:6, 2] - v[4:6, 0])[:, 2] < 0)
        assert len(c.cs.lights) == 3
        tiles = [(0, 0, c.W, c.H)]
        for depth in (0, 5):
            for form in FORMS:
                rad = c.check(form, depth, tiles, "simple")
                c.check(form, depth, tiles, "simple", count=1)
            if depth == 0:   # only the double-sided emitter shows: blue above red, nothing of the first one's colour
                lit = rad[rad.sum(axis=2) > 0]
                assert len(lit) > 0 and np.all(lit[:, 2] > lit[:, 0])


def one_step_scenes():
    ct = scene.ConstantTexture
    rng = np.random.default_rng(7)
    img = lambda h, w, k=1.0: scene.ImageTexture(rng.random((h, w, 4), dtype=np.float32) * np.float32(k))
    out = {}
    sc = cornell((32, 32))
    sc.shapes[0].materials[6] = scene.MixMaterial(ct([0.3, 0.3, 0.3]), scene.DiffuseMaterial(ct([0.2, 0.7, 0.2])),
                                                  scene.DiffuseMaterial(ct([0.7, 0.2, 0.2])))
    out["mix"] = sc
    sc = cornell((32, 32))
    sc.shapes[0].materials[5] = scene.GlossyMaterial(ct([0.9, 0.8, 0.7]), ct([0.4, 0.4, 0.4]))
    out["glossy"] = sc
    sc = cornell((32, 32))
    sc.shapes[0].materials[0] = scene.DiffuseMaterial(img(23, 37))
    out["diffuse_image"] = sc
    sc = cornell((32, 32))
    sc.shapes[0].materials[7] = scene.EmissiveMaterial(img(4, 6, 20.0))
    out["emission_image"] = sc
    return out


@pytest.mark.parametrize("name", ["mix", "glossy", "diffuse_image", "emission_image"])
def test_one_step_from_simple_runs_the_general_build(hip_ctx_factory, name):
    with hip_ctx_factory(0) as ctx:
        c = Case(ctx, one_step_scenes()[name])
        for form in FORMS:
            for tab in (0, 1):
                rad = c.check(form, 5, [(0, 0, c.W, c.H)], "general", tab=tab)
        assert rad.mean() > 0
        c.check("k_path", 5, [(0, 0, c.W, c.H)], "general", count=1)


def test_the_build_follows_the_committed_scene(hip_ctx_factory):
    """One context, four commits' worth of renders: the flag is the committed tables', never the last scene's."""
    tiles = [(0, 0, 32, 32)]
    with hip_ctx_factory(0) as ctx:
        assert ctx.render_info()["shading"] is None          # nothing rendered
        c = Case(ctx, cornell((32, 32)))
        c.check("k_path", 5, tiles, "simple")
        for name, form in (("emission_image", "k_path"), ("glossy", "k_path_spec")):
            ctx.clear_meshes()
            c = Case(ctx, one_step_scenes()[name])
            c.check(form, 5, tiles, "general")
        ctx.clear_meshes()
        c = Case(ctx, cornell((32, 32)))
        for k, v in FORMS["k_path"].items():
            ctx.set_option(k, v)
        rad, w = ctx.render(2, 5, tiles, 32, 32)
        assert ctx.render_info()["shading"] == "simple"
        c.compare(rad, w, 2, 5, tiles, "simple scene again")
        rad, w = ctx.render_continue(1, 32, 32)
        assert ctx.render_form()["form"] == "k_path" and ctx.render_info()["shading"] == "simple"
        c.compare(rad, w, 3, 5, tiles, "its continued render")
        # the wavefront kernels shade with the general build
        ctx.set_option("path", 0)
        rad, w = ctx.render(2, 5, tiles, 32, 32)
        assert ctx.render_form()["form"] == "wavefront" and ctx.render_info()["shading"] == "general"
        c.compare(rad, w, 2, 5, tiles, "wavefront", count=None)

"""The environment light on the device against its restatement.

tests/golden/env_restate.py states the definition in numpy f32; tests/golden/make_env_golden.py ran it
into env_kat.json (function vectors) and env_golden_<scene>.npz (per-pixel results, brute-force
intersection, empty ambiguity masks).  The device has to give the same bits: the unit entry points
against the vectors, and every golden scene in film, weight, final sampler state and (counting build)
closest-hit and shadow ray counts, whatever options, builder, session split or context split is used.
"""
import json
import sys

import numpy as np
import pytest

from akari_amd import capi, render, scene
from conftest import CORNELL_MESH, GOLDEN
from test_gpu_path_kat import probe_frame
from test_path_kat_host import M, check, compare_with_golden, f32, golden

sys.path.insert(0, str(GOLDEN))
import make_env_golden as ME  # noqa: E402

pytestmark = pytest.mark.gpu

KAT = json.loads((GOLDEN / "env_kat.json").read_text())


def env_golden(name):
    return np.load(GOLDEN / f"env_golden_{name}.npz")


def upload(ctx, name, select_prob=0.5, **build_kw):
    cs = scene.compile_scene(ME.build_scene(name, select_prob=select_prob))
    scene.upload_scene(ctx, cs, **build_kw)
    return cs


def render_and_compare(ctx, name, what, counting=False, exact_cull=False):
    """Every configuration of the scene; the select_prob of a configuration is part of the upload."""
    g = env_golden(name)
    H, W = g["mask"].shape
    assert not g["mask"].any()
    ctx.set_option("pixel_probe", 1)
    ctx.set_option("count_tests", int(counting))
    try:
        sp_now = None
        for key, sp, depth, clamp in ME.CONFIGS[name]:
            if sp != sp_now:
                cs = scene.compile_scene(ME.build_scene(name, select_prob=sp))
                scene.upload_environment(ctx, cs.environment)
                sp_now = sp
            rad, w = ctx.render(ME.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp, exact_cull=exact_cull)
            rays = compare_with_golden(g, key, g["mask"], rad, w, probe_frame(ctx, W, H), f"{name} {key} {what}")
            assert ctx.render_form()["form"] == "wavefront", ctx.render_form()
            if counting:
                assert rays, f"{what}: the counting build recorded no ray counts"
    finally:
        ctx.set_option("count_tests", 0)
        ctx.set_option("pixel_probe", 0)


@pytest.mark.parametrize("tag", list(ME.KAT_MAPS))
def test_unit_entry_points_equal_vectors(hip_ctx_factory, tag):
    k = KAT[tag]
    s = ME.kat_env(tag)
    with hip_ctx_factory(0) as ctx:
        with pytest.raises(capi.AkrError, match="no environment light"):
            ctx.environment_eval(f32(k["dirs"], 3))
        ctx.upload_environment(s["map"], s["scale"], 0.5, np.ascontiguousarray(s["M"].T))
        rgb, pdf = ctx.environment_eval(f32(k["dirs"], 3))
        check(rgb, f32(k["eval_rgb"], 3), f"{tag} eval texel")
        check(pdf, f32(k["eval_pdf"]), f"{tag} eval pdf")
        d, rgb, pdf = ctx.environment_sample(f32(k["u"], 2))
        check(pdf, f32(k["sample_pdf"]), f"{tag} sample pdf")
        check(rgb, f32(k["sample_rgb"], 3), f"{tag} sampled texel")
        live = ~(f32(k["sample_pdf"]) <= 0)     # a direction is defined where the pdf is positive
        check(d[live], f32(k["sample_dir"], 3)[live], f"{tag} sample direction")
        ctx.upload_environment(None)
        with pytest.raises(capi.AkrError, match="no environment light"):
            ctx.environment_sample(f32(k["u"], 2))


@pytest.mark.parametrize("name", list(ME.CONFIGS))
def test_scenes_equal_golden_default_options(hip_ctx_factory, name):
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        render_and_compare(ctx, name, "default options")
        render_and_compare(ctx, name, "default options, counting build", counting=True)


@pytest.mark.parametrize("name", list(ME.CONFIGS))
def test_scenes_equal_golden_path_forced_and_exact_cull(hip_ctx_factory, name):
    """`path` 1 asks for the persistent kernel; with an environment the wavefront form runs and says so."""
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name)
        for k, v in {"path": 1, "path_defer": 0, "path_spec": 0}.items():
            ctx.set_option(k, v)
        render_and_compare(ctx, name, "path 1 forced")
        render_and_compare(ctx, name, "path 1 forced, counting build", counting=True)
        ctx.set_option("path", 2)
        render_and_compare(ctx, name, "exact_cull", exact_cull=True)


@pytest.mark.parametrize("builder", ["sbvh", "lbvh"])
@pytest.mark.parametrize("name", list(ME.CONFIGS))
def test_builders_equal_golden(hip_ctx_factory, name, builder):
    kw = {"sbvh": dict(builder=capi.BUILDER_SBVH), "lbvh": dict(builder=capi.BUILDER_LBVH)}[builder]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, **kw)
        render_and_compare(ctx, name, builder)


def test_continue_two_plus_two_equals_four(hip_ctx_factory):
    name, (key, sp, depth, clamp) = "cornell", ME.CONFIGS["cornell"][2]
    g = env_golden(name)
    H, W = g["mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, sp)
        ctx.set_option("pixel_probe", 1)
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        rad, w = ctx.render_continue(2, W, H)
        # (the probe's ray counts are those of the last segment alone, so they are not compared here)
        check(rad, g[key + "_radiance"], "2 + 2 spp by render_continue: radiance")
        check(w, g[key + "_weight"], "2 + 2 spp by render_continue: weight")
        assert np.array_equal(probe_frame(ctx, W, H)["seed"], g[key + "_seed"]), "2 + 2 spp: final sampler states"
        # an upload ends the session, the environment's like every other
        scene.upload_environment(ctx, scene.compile_scene(ME.build_scene(name)).environment)
        with pytest.raises(capi.AkrError, match="no render session to continue"):
            ctx.render_continue(1, W, H)
        ctx.render(1, depth, [(0, 0, W, H)], W, H)
        ctx.upload_environment(None)
        with pytest.raises(capi.AkrError, match="no render session to continue"):
            ctx.render_continue(1, W, H)


def test_two_context_split_equals_single(hip_ctx_factory):
    name, (key, sp, depth, clamp) = "sky", ME.CONFIGS["sky"][1]
    g = env_golden(name)
    H, W = g["mask"].shape
    tiles = [(x, y, x + 8, y + 8) for y in range(0, H, 8) for x in range(0, W, 8)]
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        upload(a, name, sp)
        upload(b, name, sp)
        rad, w = capi.render_node([a, b], ME.SPP, depth, tiles, W, H, ray_clamp=clamp)
        check(rad, g[key + "_radiance"], "two-context render_node radiance")
        check(w, g[key + "_weight"], "two-context render_node weight")


def test_upload_then_clear_gives_todays_bits(hip_ctx_factory):
    """Without an environment every bit and every draw is what it was: the Cornell golden of the path
    loop's restatement, after an environment was set and removed again."""
    g = golden("cornell")
    H, W = g["mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "cornell")
        ctx.render(1, 2, [(0, 0, W, H)], W, H)
        ctx.upload_environment(None)
        ctx.set_option("pixel_probe", 1)
        for depth, clamp in M.CONFIGS["cornell"]:
            rad, w = ctx.render(M.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
            compare_with_golden(g, M.cfg_key(depth, clamp), g["mask"], rad, w, probe_frame(ctx, W, H),
                                f"cornell depth {depth} after the environment was removed")


def test_sampler_edge_pixels(hip_ctx_factory):
    """Pixels of a 65535 x 65535 camera whose seed makes su.x exactly select_prob (the area lights are
    taken, with a remapped draw of 0), or the environment's lu.x / lu.y exactly 0; each a one-pixel tile."""
    torch = pytest.importorskip("torch")
    e = np.load(GOLDEN / "env_golden_edges.npz")
    assert set(e["role"].tolist()) == {"light_select", "env_ux", "env_uy"}
    W, spp, depth = (int(v) for v in e["params"])
    for name in sorted(set(e["scene"].tolist())):
        idx = np.nonzero(e["scene"] == name)[0]
        tiles = [(int(x), int(y), int(x) + 1, int(y) + 1) for x, y in e["xy"][idx]]
        with hip_ctx_factory(0) as ctx:
            scene.upload_scene(ctx, scene.compile_scene(ME.build_scene(name, (W, W))))
            ctx.set_option("pixel_probe", 1)
            for counting in (0, 1):
                ctx.set_option("count_tests", counting)
                rad = torch.zeros(len(idx) * 3, device="cuda:0")
                wt = torch.zeros(len(idx), device="cuda:0")
                assert ctx.render_device(spp, depth, tiles, rad.data_ptr(), wt.data_ptr()) == len(idx)
                ctx.synchronize()
                what = f"{name} pixels {e['role'][idx].tolist()}"
                check(rad.cpu().numpy().reshape(-1, 3), e["radiance"][idx], what + " radiance")
                check(wt.cpu().numpy(), e["weight"][idx], what + " weight")
                pr = ctx.pixel_probe(len(idx))
                assert np.array_equal(pr["seed"], e["seed"][idx]), what + " final sampler state"
                if counting:
                    assert np.all(pr["flags"] & capi.PROBE_RAYS)
                    assert np.array_equal(pr["closest_rays"], e["closest"][idx]), what
                    assert np.array_equal(pr["shadow_rays"], e["shadow"][idx]), what
            ctx.set_option("count_tests", 0)


def test_library_refusals(hip_ctx_factory):
    good = np.ones((4, 4, 3), np.float32)
    with hip_ctx_factory(0) as ctx:
        def refused(match, m=good, **kw):
            with pytest.raises(capi.AkrError, match=match):
                ctx.upload_environment(m, **kw)
        with pytest.raises(capi.AkrError, match="resolution"):      # N = 0 (the binding's own check aside)
            ctx._check(ctx.lib.akr_hip_upload_environment(ctx.h, capi.C.byref(capi.Environment(0, 0)), capi._ptr(good)))
        neg, black = good.copy(), np.zeros((4, 4, 3), np.float32)
        neg[2, 1, 2] = -1.0
        refused("negative or not finite", neg)
        neg[2, 1, 2] = np.inf
        refused("negative or not finite", neg)
        refused("zero everywhere", black)
        refused("zero everywhere", good, scale=(0.0, 0.0, 0.0))
        refused("select_prob", good, select_prob=0.0)
        refused("select_prob", good, select_prob=1.0)
        refused("resolution", np.ones((2049, 2049, 3), np.float32))
        with pytest.raises(capi.AkrError, match="no environment light"):   # a refused upload sets nothing
            ctx.environment_eval(np.array([[0, 1, 0]], np.float32))


SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: Path {{ spp: 4, max_depth: 3, tile_size: 16 }},
    output: "{out}",
    environment: EnvironmentLight {{ image: "sky.pfm", scale: [1.5, 1.5, 2], rotation: [0, 30, 0], resolution: 16 }},
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, $grey, $grey, $grey] }} ]
}}
"""


def test_cli_environment_from_pfm_with_denoise(tmp_path):
    """A .akari file whose only light is an EnvironmentLight read from a lat-long .pfm."""
    from akari_amd import film
    sky = np.zeros((8, 16, 3), np.float32)
    sky[:4] = [0.4, 0.6, 1.0]
    sky[4:] = [0.1, 0.1, 0.1]
    sky[1, 3] = [300.0, 280.0, 250.0]
    film.write_pfm(tmp_path / "sky.pfm", sky, np.ones(sky.shape[:2], np.float32))
    out = tmp_path / "o.pfm"
    (tmp_path / "s.akari").write_text(SDL.format(out=out, mesh=CORNELL_MESH))
    assert render.main([str(tmp_path / "s.akari"), "--denoise"]) == 0
    from akari_amd import envmap
    img = envmap.read_pfm(out)
    assert img.shape == (24, 40, 3) and np.all(np.isfinite(img)) and img.mean() > 0

"""Mirror and Glass on the device against their restatement.

tests/golden/specular_restate.py states the two closures and the path loop's via_delta rule in numpy f32;
tests/golden/make_specular_golden.py ran it into specular_golden_<scene>.npz, every configuration with `mis`
off and on.  The device has to give the same bits in film, weight, final sampler state and (counting build)
closest-hit and shadow ray counts, whatever options, builder, session split or context split is used, and a
scene that holds either material renders in the wavefront form whatever `path` says.
"""
import subprocess
import sys

import numpy as np
import pytest

from akari_amd import capi, progressive, render, scene
from conftest import CORNELL_MESH, GOLDEN, ROOT
from test_gpu_path_kat import probe_frame
from test_path_kat_host import M, check, compare_with_golden, golden

sys.path.insert(0, str(GOLDEN))
import make_specular_golden as MS  # noqa: E402
import ref_restate as R  # noqa: E402
import specular_restate as S  # noqa: E402
import specular_scenes  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = list(MS.CONFIGS)
PATH_FORCED = {"path": 1, "path_defer": 0, "path_spec": 0}


def spec_golden(name):
    return np.load(GOLDEN / f"specular_golden_{name}.npz")


def upload(ctx, name, key, **build_kw):
    cs = scene.compile_scene(MS.build_scene(name, key))
    scene.upload_scene(ctx, cs, **build_kw)
    return cs


def config(name, key):
    return next(c for c in MS.CONFIGS[name] if c[0] == key)


def render_and_compare(factory, name, what, counting=(0,), exact_cull=False, options=None, **build_kw):
    """Every configuration of the scene, `mis` off and on, each configuration in a context of its own (a context
    holds one scene); `counting`: the values of count_tests to render with."""
    g = spec_golden(name)
    for key, _, _, _, depth, clamp in MS.CONFIGS[name]:
        with factory(0) as ctx:
            for k, v in (options or {}).items():
                ctx.set_option(k, v)
            ctx.set_option("pixel_probe", 1)
            upload(ctx, name, key, **build_kw)
            for mis in (0, 1):
                gk = key + ("_mis" if mis else "")
                mask = g[gk + "_mask"]
                H, W = mask.shape
                ctx.set_option("mis", mis)
                for c in counting:
                    ctx.set_option("count_tests", c)
                    rad, w = ctx.render(MS.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp, exact_cull=exact_cull)
                    rays = compare_with_golden(g, gk, mask, rad, w, probe_frame(ctx, W, H), f"{name} {gk} {what} count {c}")
                    assert ctx.render_form()["form"] == "wavefront", ctx.render_form()
                    if c:
                        assert rays, f"{what}: the counting build recorded no ray counts"


@pytest.mark.parametrize("name", SCENES)
def test_scenes_equal_golden_default_options(hip_ctx_factory, name):
    render_and_compare(hip_ctx_factory, name, "default options", counting=(0, 1))


@pytest.mark.parametrize("name", SCENES)
def test_scenes_equal_golden_path_forced_and_exact_cull(hip_ctx_factory, name):
    """`path` 1 asks for the persistent kernel; a specular scene runs the wavefront form and says so."""
    render_and_compare(hip_ctx_factory, name, "path 1 forced", options=PATH_FORCED)
    render_and_compare(hip_ctx_factory, name, "exact_cull", exact_cull=True)


@pytest.mark.parametrize("builder", ["sbvh", "lbvh"])
@pytest.mark.parametrize("name", SCENES)
def test_builders_equal_golden(hip_ctx_factory, name, builder):
    kw = {"sbvh": dict(builder=capi.BUILDER_SBVH), "lbvh": dict(builder=capi.BUILDER_LBVH)}[builder]
    render_and_compare(hip_ctx_factory, name, builder, **kw)


@pytest.mark.parametrize("mis", [0, 1])
def test_continue_and_film_variance_change_no_bit(hip_ctx_factory, mis):
    name, (key, _, _, _, depth, clamp) = "glass_box", MS.CONFIGS["glass_box"][0]
    g, gk = spec_golden(name), key + ("_mis" if mis else "")
    H, W = g[gk + "_mask"].shape
    with hip_ctx_factory(0) as ctx:
        upload(ctx, name, key)
        ctx.set_option("pixel_probe", 1)
        ctx.set_option("mis", mis)
        ctx.render(2, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        rad, w = ctx.render_continue(2, W, H)
        assert ctx.render_form()["form"] == "wavefront"
        check(rad, g[gk + "_radiance"], "2 + 2 spp by render_continue: radiance")
        check(w, g[gk + "_weight"], "2 + 2 spp by render_continue: weight")
        assert np.array_equal(probe_frame(ctx, W, H)["seed"], g[gk + "_seed"]), "2 + 2 spp: final sampler states"
        ctx.set_option("film_variance", 1)
        rad, w = ctx.render(MS.SPP, depth, [(0, 0, W, H)], W, H, ray_clamp=clamp)
        compare_with_golden(g, gk, g[gk + "_mask"], rad, w, probe_frame(ctx, W, H), "film_variance on")
        assert ctx.render_variance(W, H).shape == (H, W, 4)


@pytest.mark.parametrize("mis", [False, True])
def test_two_context_split_equals_single(hip_ctx_factory, mis):
    name, key = "sky_spec", "area_d4"
    _, _, _, _, depth, clamp = config(name, key)
    g, gk = spec_golden(name), key + ("_mis" if mis else "")
    H, W = g[gk + "_mask"].shape
    tiles = [(x, y, x + 8, y + 8) for y in range(0, H, 8) for x in range(0, W, 8)]
    with hip_ctx_factory(0) as a, hip_ctx_factory(0) as b:
        upload(a, name, key)
        upload(b, name, key)
        rad, w = capi.render_node([a, b], MS.SPP, depth, tiles, W, H, ray_clamp=clamp, mis=mis)
        check(rad, g[gk + "_radiance"], "two-context render_node radiance")
        check(w, g[gk + "_weight"], "two-context render_node weight")


def test_shallow_render_after_a_deep_one(hip_ctx_factory):
    """max_depth 1 after a deep render in the same context: a terminal term E or a via_delta flag left by the deep
    render's passes must not reach it.  Both with the flag queue (mis off) and with the carried record (mis on)."""
    name = "mirror_box"
    g = spec_golden(name)
    H, W = g["d1_mask"].shape
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        upload(ctx, name, "d1")
        for mis in (0, 1):
            ctx.set_option("mis", mis)
            gk = "d1" + ("_mis" if mis else "")
            ctx.render(MS.SPP + 1, 5, tiles, W, H)      # terminal terms and flags in both parities
            rad, w = ctx.render(MS.SPP, 1, tiles, W, H)
            compare_with_golden(g, gk, g[gk + "_mask"], rad, w, probe_frame(ctx, W, H), f"d1 after d5, mis {mis}")
            rad, w = ctx.render(MS.SPP, 0, tiles, W, H)  # camera rays alone: what path_golden_cornell's d0 holds
            gp = golden("cornell")
            check(rad, gp["d0_radiance"], f"d0 after d5, mis {mis}: the plain box's camera-ray film")


def test_plain_scene_after_a_specular_one_is_todays(hip_ctx_factory):
    """akr_hip_clear_meshes, then the unmodified Cornell box on the same context: has_specular follows the
    committed scene, so the persistent form runs again and gives the existing golden's bits."""
    gp = golden("cornell")
    H, W = gp["mask"].shape
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        ctx.set_option("pixel_probe", 1)
        for k, v in PATH_FORCED.items():
            ctx.set_option(k, v)
        upload(ctx, "mixed_spec", "d5")
        ctx.render(MS.SPP, 5, tiles, W, H)
        assert ctx.render_form()["form"] == "wavefront"
        ctx.clear_meshes()
        scene.upload_scene(ctx, scene.compile_scene(M.build_scene("cornell")))
        rad, w = ctx.render(M.SPP, 5, tiles, W, H)
        assert ctx.render_form()["form"] == "k_path", ctx.render_form()
        compare_with_golden(gp, "d5", gp["mask"], rad, w, probe_frame(ctx, W, H), "cornell after a specular scene")


# ----------------------------------------------------------------------------- per-slot counts
_PREFIX = {}


def sky_prefixes(cap):
    """The restatement's `sky_spec` area_d4 film sums and sampler states after 1 .. cap samples of every pixel,
    run once: a slot's samples are one chain, so a slot that holds c samples equals entry c."""
    if cap not in _PREFIX:
        _, _, _, _, depth, _ = config("sky_spec", "area_d4")
        sc = S.SpecScene(MS.build_scene("sky_spec", "area_d4"))
        env = MS.restated_env()
        W, H = sc.camera.res
        film = np.zeros((cap + 1, H, W, 3), np.float32)
        seed = np.zeros((cap + 1, H, W), np.uint32)
        for y in range(H):
            for x in range(W):
                sampler, tr, rad = R.LCG(x + y * W), R.Tracer(sc), (R.F(0.0),) * 3
                seed[0, y, x] = sampler.seed
                for c in range(1, cap + 1):
                    L = S.path_sample(sc, sampler, x, y, depth, None, tr, None, None, env, False)
                    rad = R.add(rad, L)
                    film[c, y, x], seed[c, y, x] = rad, sampler.seed
        film.setflags(write=False)
        seed.setflags(write=False)
        _PREFIX[cap] = (film, seed, depth)
    return _PREFIX[cap]


def check_per_slot(ctx, film, seed, w, rad, what):
    H, W = w.shape
    count = w.astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    check(rad, film[count, ys, xs], f"{what}: radiance per slot count")
    sampler, sfilm = ctx.render_state_export()
    assert np.array_equal(sfilm[:, 3].reshape(H, W), w), f"{what}: exported weights"
    assert np.array_equal(sampler.reshape(H, W), seed[count, ys, xs]), f"{what}: sampler states per slot count"
    return count


def test_masked_continue_and_stepwise_adaptive_equal_restatement_per_slot(hip_ctx_factory):
    cap = 6
    film, seed, depth = sky_prefixes(cap)
    H, W = seed.shape[1:]
    tiles = [(0, 0, W, H)]
    with hip_ctx_factory(0) as ctx:
        upload(ctx, "sky_spec", "area_d4")
        ctx.render(2, depth, tiles, W, H)
        mask = (np.arange(W * H) % 3 == 0).astype(np.uint8)
        rad, w = ctx.render_continue_masked(2, mask, W, H)
        assert ctx.render_form()["form"] == "wavefront"
        count = check_per_slot(ctx, film, seed, w, rad, "masked continue")
        assert np.array_equal(count.reshape(-1), np.where(mask != 0, 4, 2))
        rad, w = ctx.render_continue(1, W, H)
        check_per_slot(ctx, film, seed, w, rad, "uniform continue of a masked session")
        rad, w, info = progressive.render_adaptive(ctx, cap, depth, tiles, W, H, 0.05, min_spp=2, pass_spp=2)
        count = check_per_slot(ctx, film, seed, w, rad, "stepwise adaptive")
        assert info["samples"] == count.sum() and count.min() >= 2 and count.max() <= cap


# ----------------------------------------------------------------------------- features
def test_feature_albedo_of_the_two_blocks(hip_ctx_factory):
    """One feature sample per pixel: where the camera ray meets the Mirror or the Glass block the albedo is the
    material's colour.  The hit of every pixel's first camera ray is the restatement's."""
    desc = specular_scenes.mirror_glass_box((24, 24))
    sc = S.SpecScene(desc)
    W, H = sc.camera.res
    with hip_ctx_factory(0) as ctx:
        scene.upload_scene(ctx, scene.compile_scene(desc))
        ft = ctx.render_features(1, [(0, 0, W, H)], W, H)
    seen = {"mirror": 0, "glass": 0}
    tr = R.Tracer(sc)
    for y in range(H):
        for x in range(W):
            sampler = R.LCG(x + y * W)
            u1, u2 = sampler.next2d(), sampler.next2d()
            o, d = sc.camera.generate_ray(u1, u2, (x, y))
            hit = tr.intersect(o, d, R.EPS, R.INF)
            mat = sc.tris[hit[0]].material if hit is not None else None
            if mat is not None and mat[0] in seen:
                seen[mat[0]] += 1
                assert np.array_equal(ft[y, x, :3], np.array(mat[1][1], np.float32)), (x, y, mat[0], ft[y, x, :4])
                assert ft[y, x, 3] == 1
    assert seen["mirror"] > 10 and seen["glass"] > 10, seen


# ----------------------------------------------------------------------------- CLI, adapter
SDL = """
let grey = DiffuseMaterial {{ color: [0.725, 0.71, 0.68] }}
let lamp = EmissiveMaterial {{ color: [17, 12, 4] }}
let mirror = MirrorMaterial {{ color: [0.9, 0.9, 0.9] }}
let glass = GlassMaterial {{ color: [1, 1, 1], ior: 1.5 }}
export scene = Scene {{
    camera: PerspectiveCamera {{ fov: 15, position: [0, 1, 9], resolution: [40, 24] }},
    integrator: Path {{ spp: 4, max_depth: 5, tile_size: 16 }},
    output: "{out}",
    shapes: [ AkariMesh {{ path: "{mesh}", materials: [$grey, $grey, $grey, $grey, $grey, ${short}, ${tall}, $lamp] }} ]
}}
"""


def test_cli_renders_mirror_and_glass(tmp_path):
    from akari_amd import envmap
    imgs = []
    for short, tall in (("grey", "grey"), ("glass", "mirror")):
        out = tmp_path / f"o_{short}.pfm"
        (tmp_path / "s.akari").write_text(SDL.format(out=out, mesh=CORNELL_MESH, short=short, tall=tall))
        assert render.main([str(tmp_path / "s.akari")]) == 0
        imgs.append(envmap.read_pfm(out))
    assert imgs[1].shape == (24, 40, 3) and np.all(np.isfinite(imgs[1])) and imgs[1].mean() > 0
    assert not np.array_equal(imgs[0], imgs[1]), "the two materials changed nothing"


def test_cpp_adapter_specular_demo(tmp_path):
    exe = tmp_path / "specular_demo"
    lib = capi.LIB_PATH.parent
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", str(ROOT / "tests" / "cpp" / "specular_demo.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lakr_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "form_wavefront=1 mirror_shows_lamp=1 bad_ior_refused=1" in r.stdout
